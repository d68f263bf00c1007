// mpcmp_motion_planner.hpp — header-only C++ mirror of the reference's planner façade over the mpcmp C ABI.
//
// Same class name, member names, argument meaning and error behaviour as `MotionPlanner`
// (mpc_solver/motionPlanner.hpp:16-176, mpc_solver/motionPlanner.cpp) and the limits table of `PandaWrapper`
// (robot_utils/pandaWrapper.hpp:28-40), so that examples/offline_trajectory.cpp / examples/benchmark.cpp keep
// their call sequence; the solve runs on the GPU through libmpcmp.so.  Additions: `solve_batch` (B problems in
// one call — what examples/benchmark.cpp:16 loops over) and the text writers of the two result formats.
//
// With Eigen on the include path the vector/matrix arguments are Eigen types exactly as in the reference;
// without it (this image has no Eigen) a minimal column-major fixed-size matrix with the same element access
// stands in.  Differences that cannot be hidden: Ruckig is replaced by the library's own jerk-limited, time-synchronised
// generator (same problem statement; it reproduces the reference's stored Ruckig trajectory), `mpc` (the polympc object)
// does not exist.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "mpcmp.h"

#if defined(MPCMP_USE_EIGEN) || (defined(__has_include) && __has_include(<Eigen/Dense>))
#include <Eigen/Dense>
namespace mpcmp_shim {
template <int R, int C> using Mat = Eigen::Matrix<double, R, C>;
}
#else
namespace mpcmp_shim {
template <int R, int C>
struct Mat {                                  // column-major like Eigen's default
    std::array<double, (size_t)R * C> d{};
    double &operator()(int i, int j) { return d[(size_t)j * R + i]; }
    double operator()(int i, int j) const { return d[(size_t)j * R + i]; }
    double &operator()(int i) { return d[i]; }
    double operator()(int i) const { return d[i]; }
    double &operator[](int i) { return d[i]; }
    double operator[](int i) const { return d[i]; }
    double *data() { return d.data(); }
    const double *data() const { return d.data(); }
    static Mat Zero() { return Mat(); }
    static constexpr int rows() { return R; }
    static constexpr int cols() { return C; }
};
}  // namespace mpcmp_shim
#endif

#define NDOF 7   // robot_utils/pandaWrapper.hpp:10

// Minimal stand-ins for the Pinocchio objects a reference caller touches through `planner.robot`
// (examples/benchmark.cpp:108-110,154-156: forwardKinematics(model, data, q); updateFramePlacement(model, data, frame_id);
//  data.oMf[frame_id].translation()[2]).  Only what those call sites use exists.
namespace mpcmp_shim {
struct Placement {
    double t[3] = {0, 0, 0};
    double Rm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double *translation() const { return t; }
    const double *rotation() const { return Rm; }          // row-major
};
struct FrameData {
    static constexpr int JOINT7 = 7, LINK8 = 8, TOOL = 9;  // oMf indices: joint-7 origin, panda_link8, panda_tool
    Placement oMf[10];
    Placement oMi[8];                                       // oMi[7]: joint-7 placement (motionPlanner.cpp:111)
};
}  // namespace mpcmp_shim
#if !(defined(__has_include) && __has_include(<pinocchio/algorithm/kinematics.hpp>))
namespace pinocchio {
// joint placements of the chain for configuration q[7] (pinocchio::forwardKinematics)
inline void forwardKinematicsArray(const mpcmp_model &model, mpcmp_shim::FrameData &data, const double *q) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    for (int i = 0; i < 7; i++) {
        for (int r = 0; r < 3; r++) p[r] += R[3 * r] * model.p[i][0] + R[3 * r + 1] * model.p[i][1] + R[3 * r + 2] * model.p[i][2];
        const double c = std::cos(q[i]), s = std::sin(q[i]);
        double J[9], Rn[9];
        for (int r = 0; r < 3; r++) {
            J[3 * r] = model.R0[i][3 * r] * c + model.R0[i][3 * r + 1] * s;
            J[3 * r + 1] = -model.R0[i][3 * r] * s + model.R0[i][3 * r + 1] * c;
            J[3 * r + 2] = model.R0[i][3 * r + 2];
        }
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++)
            Rn[3 * r + k] = R[3 * r] * J[k] + R[3 * r + 1] * J[3 + k] + R[3 * r + 2] * J[6 + k];
        for (int k = 0; k < 9; k++) R[k] = Rn[k];
        for (int k = 0; k < 3; k++) data.oMi[i + 1].t[k] = p[k];
        for (int k = 0; k < 9; k++) data.oMi[i + 1].Rm[k] = R[k];
    }
}
template <class V> inline void forwardKinematics(const mpcmp_model &model, mpcmp_shim::FrameData &data, const V &q) {
    double qq[7];
    for (int j = 0; j < 7; j++) qq[j] = q(j);
    forwardKinematicsArray(model, data, qq);
}
// placement of one operational frame from the joint placements (pinocchio::updateFramePlacement)
inline void updateFramePlacement(const mpcmp_model &model, mpcmp_shim::FrameData &data, int frame_id) {
    const mpcmp_shim::Placement &j7 = data.oMi[7];
    const double *off = frame_id == mpcmp_shim::FrameData::TOOL ? model.tool : (frame_id == mpcmp_shim::FrameData::LINK8 ? model.link8 : nullptr);
    mpcmp_shim::Placement &f = data.oMf[frame_id];
    for (int k = 0; k < 9; k++) f.Rm[k] = j7.Rm[k];
    for (int r = 0; r < 3; r++)
        f.t[r] = j7.t[r] + (off ? j7.Rm[3 * r] * off[0] + j7.Rm[3 * r + 1] * off[1] + j7.Rm[3 * r + 2] * off[2] : 0.0);
}
}  // namespace pinocchio
#endif

// limits table + model of robot_utils/pandaWrapper.hpp (Pinocchio members replaced by mpcmp_model)
class PandaWrapper {
  public:
    using Vec7 = mpcmp_shim::Mat<NDOF, 1>;
    mpcmp_model model;
    mpcmp_shim::FrameData data;                                   // robot_utils/pandaWrapper.hpp:19 (pinocchio::Data)
    int frame_id = mpcmp_shim::FrameData::TOOL;                   // getFrameId("panda_tool"), pandaWrapper.cpp:11
    Vec7 min_position, max_position, max_velocity, max_acceleration, max_jerk, max_torque;
    double max_torqueDot{1000};
    double max_linear_velocity{1.7};
    double max_angular_velocity{2.5};
    double min_height{0.05};
    explicit PandaWrapper(const std::string &urdf_path) {
        const int rc = urdf_path.empty() ? mpcmp_default_model(&model) : mpcmp_model_from_urdf(urdf_path.c_str(), &model);
        if (rc) throw std::runtime_error(std::string("PandaWrapper: ") + mpcmp_last_error(nullptr));
        mpcmp_default_limits(min_position.data(), max_position.data(), max_velocity.data(), max_acceleration.data(),
                             max_jerk.data(), max_torque.data());
    }
    // world position of the joint-7 origin (oMi[7]) and of the tool frame
    void forward_kinematics(const double *q, double *p_joint7, double *p_tool) const {
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
        for (int i = 0; i < 7; i++) {
            for (int r = 0; r < 3; r++) p[r] += R[3 * r] * model.p[i][0] + R[3 * r + 1] * model.p[i][1] + R[3 * r + 2] * model.p[i][2];
            const double c = std::cos(q[i]), s = std::sin(q[i]);
            double J[9], Rn[9];
            for (int r = 0; r < 3; r++) {
                J[3 * r] = model.R0[i][3 * r] * c + model.R0[i][3 * r + 1] * s;
                J[3 * r + 1] = -model.R0[i][3 * r] * s + model.R0[i][3 * r + 1] * c;
                J[3 * r + 2] = model.R0[i][3 * r + 2];
            }
            for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++)
                Rn[3 * r + k] = R[3 * r] * J[k] + R[3 * r + 1] * J[3 + k] + R[3 * r + 2] * J[6 + k];
            for (int k = 0; k < 9; k++) R[k] = Rn[k];
        }
        if (p_joint7) for (int r = 0; r < 3; r++) p_joint7[r] = p[r];
        if (p_tool) for (int r = 0; r < 3; r++)
            p_tool[r] = p[r] + R[3 * r] * model.tool[0] + R[3 * r + 1] * model.tool[1] + R[3 * r + 2] * model.tool[2];
    }
    // robot_utils/pandaWrapper.cpp:62-88: joint velocity realising a task velocity (damped pseudo-inverse)
    Vec7 inverse_velocities(const Vec7 &q, const mpcmp_shim::Mat<3, 1> &linear_velocity, const mpcmp_shim::Mat<3, 1> &angular_velocity) const {
        Vec7 qd;
        if (mpcmp_inverse_velocities(&model, q.data(), linear_velocity.data(), angular_velocity.data(), qd.data()))
            throw std::runtime_error("PandaWrapper::inverse_velocities failed");
        return qd;
    }
    // robot_utils/pandaWrapper.cpp:90-107: [linear; angular] velocity of the tool frame, world-aligned
    mpcmp_shim::Mat<6, 1> forward_velocities(const Vec7 &q, const Vec7 &qdot) const {
        mpcmp_shim::Mat<6, 1> out;
        if (mpcmp_forward_velocities(&model, q.data(), qdot.data(), out.data())) throw std::runtime_error("PandaWrapper::forward_velocities failed");
        return out;
    }
    // robot_utils/pandaWrapper.cpp:14-60.  The reference starts from a random configuration and drops the success flag;
    // here the start is explicit (default: zeros) and `converged`, when given, receives the flag.
    Vec7 inverse_kinematic(const mpcmp_shim::Mat<3, 3> &orientation, const mpcmp_shim::Mat<3, 1> &position, const Vec7 *q_init = nullptr,
                           bool *converged = nullptr) const {
        double R[9];
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R[3 * r + c] = orientation(r, c);
        Vec7 q;
        const int rc = mpcmp_inverse_kinematics(&model, R, position.data(), q_init ? q_init->data() : nullptr, q.data(), nullptr);
        if (rc != 0 && rc != 1) throw std::runtime_error("PandaWrapper::inverse_kinematic failed");
        if (converged) *converged = rc == 0;
        return q;
    }
};

class MotionPlanner;
namespace mpcmp_shim {
// What a reference caller can reach through the public member `mpc` (motionPlanner.hpp:28-29: polympc's MPC<> object),
// reduced to the calls the facade itself makes (motionPlanner.cpp:15-20,33,47,72-97,172-174,184-207; motionPlanner.hpp:106-125):
// settings, guesses, bounds, solve, the solution and its interpolation, and the solver info.  The polympc object itself does
// not exist here: the setters write the planner's configuration record and guess, which the next solve hands to the library.
struct MpcView {
    struct Settings { int &max_iter; int &line_search_max_iter; };
    struct QpSettings { int &max_iter; double &eps_rel; double &eps_abs; };
    struct Status { int value; };
    struct InfoView { Status status; int iter; int qp_iters_total; };
    explicit MpcView(MotionPlanner *o) : owner(o) {}
    Settings settings();
    QpSettings qp_settings();
    std::array<double, 1> solution_p() const;
    const std::vector<double> &solution_x() const;
    const std::vector<double> &solution_u() const;
    Mat<2 * NDOF, 1> solution_x_at(double t) const;       // normalised time in [0,1]
    Mat<NDOF, 1> solution_u_at(double t) const;
    InfoView info() const;
    std::vector<double> time_nodes() const;                // mpc.ocp().time_nodes
    // ---- write side ----
    // guesses in the layout of solution_x() / solution_u(): node-major, node 0 = the current state (motionPlanner.cpp:172-174,205-207)
    void x_guess(const std::vector<double> &x);            // [14 N]
    void u_guess(const std::vector<double> &u);            // [7 N]
    void p_guess(const std::array<double, 1> &p);          // final time
    void p_guess(double T) { p_guess(std::array<double, 1>{T}); }
    // bounds (motionPlanner.cpp:72,75,80,97); they are overwritten by the next set_constraint_margins(), as in the reference
    void state_bounds(const Mat<2 * NDOF, 1> &lb, const Mat<2 * NDOF, 1> &ub);
    void control_bounds(const Mat<NDOF, 1> &lb, const Mat<NDOF, 1> &ub);
    void parameters_bounds(const std::array<double, 1> &lb, const std::array<double, 1> &ub);
    void constraints_bounds(const Mat<NDOF + 1, 1> &lb, const Mat<NDOF + 1, 1> &ub);      // 7 torques, tool height
    // motionPlanner.cpp:47 / :33: the solver pins the first node to the centre of the box and keeps the last node within its
    // half-width (one half-width for all 14 entries: the largest given)
    void initial_state_bounds(const Mat<2 * NDOF, 1> &lb, const Mat<2 * NDOF, 1> &ub);
    void final_state_bounds(const Mat<2 * NDOF, 1> &lb, const Mat<2 * NDOF, 1> &ub);
    void solve();                                          // motionPlanner.cpp:184, from the guess set above
  private:
    MotionPlanner *owner;
};

// Look-alikes of the three Ruckig members (motionPlanner.hpp:34-37) for callers that touch them directly: the input record
// (ruckig::InputParameter's field names), the trajectory (get_duration / at_time) and `otg.calculate(input, trajectory)`.
// Behind them is the library's jerk-limited, time-synchronised generator (mpcmp_jerk_point_lim_batch); every field of the input record is used.
enum Result { Working = 0, Finished = 1, Error = -1 };     // ruckig::Result, the values motionPlanner.cpp:149 can see
struct InputParameter {
    std::array<double, NDOF> current_position{}, current_velocity{}, current_acceleration{};
    std::array<double, NDOF> target_position{}, target_velocity{}, target_acceleration{};
    std::array<double, NDOF> max_velocity{}, max_acceleration{}, max_jerk{};
};
struct Trajectory {
    double get_duration() const { return duration; }
    // position, velocity, acceleration at min(time, duration) (ruckig::Trajectory::at_time, motionPlanner.cpp:160)
    void at_time(double time, std::array<double, NDOF> &position, std::array<double, NDOF> &velocity, std::array<double, NDOF> &acceleration) const;
  private:
    friend struct Otg;
    MotionPlanner *owner = nullptr;
    InputParameter in;
    double duration = -1.0;
};
struct Otg {
    explicit Otg(MotionPlanner *o) : owner(o) {}
    Result calculate(const InputParameter &input, Trajectory &trajectory);    // motionPlanner.cpp:149
  private:
    MotionPlanner *owner;
};
}  // namespace mpcmp_shim

class MotionPlanner {
  public:
    using Vec7 = mpcmp_shim::Mat<NDOF, 1>;
    using Vec14 = mpcmp_shim::Mat<2 * NDOF, 1>;
    using mpc_t = mpcmp_shim::MpcView;
    mpc_t mpc{this};                                                     // motionPlanner.hpp:28-29 (view, see MpcView)

    PandaWrapper robot;
    mpcmp_shim::Otg otg{this};                                           // motionPlanner.hpp:35-37 (look-alikes, see above)
    mpcmp_shim::Trajectory trajectory;
    mpcmp_shim::InputParameter input;
    Vec14 current_state, target_state;
    const double eps = 1e-2;                                            // motionPlanner.hpp:44
    const double inf = std::numeric_limits<double>::infinity();
    double margin_position_, margin_velocity_, margin_acceleration_, margin_torque_, margin_jerk_;
    mpcmp_config config;                                                 // stands in for mpc.settings()/qp_settings()
    mpcmp_info last_info{};

    // num_seg / sqp_iters default to the reference as shipped (robot_ocp.hpp:32, motionPlanner.cpp:15)
    explicit MotionPlanner(std::string urdf_path, int num_seg = 6, int sqp_iters = 2, int max_batch = 1024, int device = 0)
        : robot(urdf_path), max_batch_(max_batch) {
        mpcmp_default_config(&config, num_seg, sqp_iters);               // motionPlanner.cpp:15-20
        N_ = mpcmp_num_nodes(num_seg);
        const int rc = mpcmp_create(&config, &robot.model, device, max_batch, &ctx_);
        if (rc) throw std::runtime_error(std::string("MotionPlanner: ") + mpcmp_last_error(nullptr));
        Vec7 mid, zero = Vec7::Zero();
        for (int j = 0; j < 7; j++) mid(j) = 0.5 * (robot.max_position(j) + robot.min_position(j));  // motionPlanner.cpp:5
        set_target_state(mid, zero);
        set_current_state(mid, zero);
        set_constraint_margins(1.0, 1.0, 1.0, 1.0, 1.0);                 // motionPlanner.cpp:24
        sol_x_.assign((size_t)14 * N_, 0.0); sol_u_.assign((size_t)7 * N_, 0.0);
    }
    ~MotionPlanner() { mpcmp_destroy(ctx_); }
    MotionPlanner(const MotionPlanner &) = delete;
    MotionPlanner &operator=(const MotionPlanner &) = delete;

    void set_target_state(Vec7 target_position, Vec7 target_velocity, Vec7 target_acceleration = Vec7::Zero()) {     // motionPlanner.cpp:27-39
        for (int j = 0; j < 7; j++) {
            target_state(j) = target_position(j); target_state(7 + j) = target_velocity(j);
            input.target_position[j] = target_position(j); input.target_velocity[j] = target_velocity(j); input.target_acceleration[j] = target_acceleration(j);
        }
    }
    void set_current_state(Vec7 current_position, Vec7 current_velocity, Vec7 current_acceleration = Vec7::Zero()) {  // motionPlanner.cpp:41-54
        for (int j = 0; j < 7; j++) {
            current_state(j) = current_position(j); current_state(7 + j) = current_velocity(j);
            input.current_position[j] = current_position(j); input.current_velocity[j] = current_velocity(j); input.current_acceleration[j] = current_acceleration(j);
        }
    }
    void set_constraint_margins(double margin_position, double margin_velocity, double margin_acceleration,
                                double margin_torque, double margin_jerk) {                          // motionPlanner.cpp:56-90
        margin_position_ = margin_position; margin_velocity_ = margin_velocity; margin_acceleration_ = margin_acceleration;
        margin_torque_ = margin_torque; margin_jerk_ = margin_jerk;
        mpcmp_set_margins(&config, margin_position, margin_velocity, margin_acceleration, margin_torque);
        mpcmp_set_min_height(&config, robot.min_height);
        push_config();
        for (int j = 0; j < 7; j++) {                                    // motionPlanner.cpp:86-88
            input.max_velocity[j] = margin_velocity * robot.max_velocity(j);
            input.max_acceleration[j] = margin_acceleration * robot.max_acceleration(j);
            input.max_jerk[j] = margin_jerk * robot.max_jerk(j);
        }
    }
    void set_min_height(double min_height) { mpcmp_set_min_height(&config, min_height); push_config(); }  // :92-100
    // extension beyond the reference's members: the load the gripper carries, added to body 7 of the robot's model for every later solve and MPC
    // sample (mass [kg] >= 0; com [3] and the inertia about the COM [9, row-major] in the joint-7 frame, the frame of the tool point).  mass 0 with
    // a zero inertia is the empty gripper.  The jerk-limited guess (get_ruckig_trajectory, get_RK_point) stays the unloaded model's.
    void set_payload(double mass, const double com[3], const double I[9]) {
        mpcmp_payload p{};
        p.mass = mass;
        for (int d = 0; d < 3; d++) p.com[d] = com[d];
        for (int q = 0; q < 9; q++) p.I[q] = I[q];
        mpcmp_model check;
        if (mpcmp_model_add_payload(&robot.model, &p, &check) != MPCMP_OK) throw std::runtime_error(std::string("mpcmp: ") + mpcmp_last_error(nullptr));
        payload_ = p; has_payload_ = true; payload_rows_ = 0;
    }

    // extension beyond the reference's members: the world the plan runs in (include/mpcmp.h, clearance).  The robot is the skeleton of
    // mpcmp_link_spheres(model, sphere_radius, sphere_spacing): spheres on the lines between the joint origins, not a fitted hull.
    // n_obs == 0 removes the obstacles.
    void set_obstacles(const mpcmp_obstacle *obs, int n_obs, double sphere_radius = 0.06, double sphere_spacing = 0.08) {
        if (n_obs > 0) {
            mpcmp_sphere sph[64];
            int n = 0;
            if (mpcmp_link_spheres(&robot.model, sphere_radius, sphere_spacing, 64, sph, &n) != MPCMP_OK)
                throw std::runtime_error("mpcmp: set_obstacles: sphere radius and spacing must be > 0 and give at most 64 spheres");
            chk(mpcmp_set_robot_spheres(ctx_, 0, n, sph));
        }
        chk(mpcmp_set_obstacles(ctx_, n_obs > 0 ? 1 : 0, n_obs, obs));
    }
    // clearance record of the last solution at n_pts + 1 uniform samples (status 0: no sample closer than `margin` to anything)
    mpcmp_clearance clearance(int n_pts = 200, double margin = 0.0, int self_gap = 0) {
        mpcmp_clearance r;
        chk(mpcmp_clearance_batch(ctx_, 1, sol_x_.data(), &sol_T_, n_pts, margin, self_gap, &r));
        return r;
    }
    // certified clearance record of the last solution (include/mpcmp_clearance_cert.h): status 0 means that no clearance falls below `margin` at ANY
    // time of the plan, not only at samples; MPCMP_CLR_UNDECIDED: not decided within max_depth halvings of the num_seg n_start first intervals.
    // *cert (may be null): the lower bound d_lower of the true minimum (which lies in [d_lower, d_min]) and the work done
    mpcmp_clearance check_clearance_certified(double margin = 0.0, int self_gap = 0, int n_start = 4, int max_depth = 10,
                                              mpcmp_clearance_cert *cert = nullptr) {
        mpcmp_clearance r;
        chk(mpcmp_clearance_certified_batch(ctx_, 1, sol_x_.data(), &sol_T_, margin, self_gap, n_start, max_depth, &r, cert));
        return r;
    }
    // A voxel world (include/mpcmp_field.h): the occupancy occ [n[2]][n[1]][n[0]] of the grid `desc`, or the voxels that contain the points
    // [n_points][3]; desc == nullptr removes it.  The robot is the skeleton of set_obstacles, set again by each of these calls
    void field_spheres(double sphere_radius, double sphere_spacing) {
        mpcmp_sphere sph[64];
        int n = 0;
        if (mpcmp_link_spheres(&robot.model, sphere_radius, sphere_spacing, 64, sph, &n) != MPCMP_OK)
            throw std::runtime_error("mpcmp: voxel world: sphere radius and spacing must be > 0 and give at most 64 spheres");
        chk(mpcmp_set_robot_spheres(ctx_, 0, n, sph));
    }
    void set_voxel_world(const mpcmp_field_desc *desc, const unsigned char *occ, double sphere_radius = 0.06, double sphere_spacing = 0.08) {
        if (desc) field_spheres(sphere_radius, sphere_spacing);
        chk(mpcmp_set_field(ctx_, desc, occ));
    }
    void set_point_cloud(const mpcmp_field_desc &desc, int n_points, const double *points, double sphere_radius = 0.06, double sphere_spacing = 0.08) {
        field_spheres(sphere_radius, sphere_spacing);
        chk(mpcmp_set_field_points(ctx_, &desc, n_points, points));
    }
    // Camera frames (include/mpcmp_frame.h): the same worlds with the robot itself, seen by the camera at the posture robot_q [7] (null: no
    // filter), removed: points, pixels or occupied voxel centres within r_s + robot_pad of a skeleton sphere.  keep: added to the world in force.
    // The counts of the last of the three calls are kept in frame_stats
    mpcmp_frame_stats frame_stats = {};
    void set_point_cloud_filtered(const mpcmp_field_desc &desc, int n_points, const double *points, const double *robot_q, double robot_pad,
                                  bool keep = false, double sphere_radius = 0.06, double sphere_spacing = 0.08) {
        field_spheres(sphere_radius, sphere_spacing);
        chk(mpcmp_set_field_points_filtered(ctx_, &desc, n_points, points, robot_q, robot_pad, keep ? MPCMP_FRAME_KEEP : 0, &frame_stats));
    }
    void set_depth_image(const mpcmp_field_desc &desc, const mpcmp_camera &camera, const void *depth, int depth_type, const double *robot_q = nullptr,
                         double robot_pad = 0.0, bool keep = false, double sphere_radius = 0.06, double sphere_spacing = 0.08) {
        field_spheres(sphere_radius, sphere_spacing);
        chk(mpcmp_set_field_depth(ctx_, &desc, &camera, depth, depth_type, robot_q, robot_pad, keep ? MPCMP_FRAME_KEEP : 0, &frame_stats));
    }
    void carve_robot(const double *robot_q, double robot_pad, double sphere_radius = 0.06, double sphere_spacing = 0.08) {
        field_spheres(sphere_radius, sphere_spacing);
        chk(mpcmp_field_carve(ctx_, robot_q, robot_pad, &frame_stats));
    }
    // the grid in force and (d2 may be null) its squared distance field d2 [n[2]][n[1]][n[0]] as the GPU built it
    void voxel_field(mpcmp_field_desc *desc, unsigned *d2 = nullptr) { chk(mpcmp_get_field(ctx_, desc, d2)); }
    // clearance record of the last solution against the voxel world (`other` is the linear index of a voxel).  merge: joined with the record of
    // clearance(n_pts, margin, self_gap) by mpcmp_clearance_merge_batch; *source (may be null) is then 1 where d_min is the field's
    mpcmp_clearance check_clearance_field(int n_pts = 200, double margin = 0.0, bool merge = false, int self_gap = 0, int *source = nullptr) {
        mpcmp_clearance r;
        chk(mpcmp_clearance_field_batch(ctx_, 1, sol_x_.data(), &sol_T_, n_pts, margin, &r));
        if (source) *source = 1;
        if (merge) {
            const mpcmp_clearance a = clearance(n_pts, margin, self_gap);
            chk(mpcmp_clearance_merge_batch(ctx_, 1, &a, &r, &r, source));
        }
        return r;
    }
    // certified clearance record of the last solution against the voxel world (include/mpcmp_field_cert.h): status 0 means clear of the occupied
    // cubes by `margin` at EVERY time of the plan; `other` is the linear index of a voxel.  *cert (may be null): the certificate.  merge: both
    // records joined with those of check_clearance_certified(margin, self_gap, n_start, max_depth) by mpcmp_clearance_merge_batch and
    // mpcmp_clearance_cert_merge_batch; *source (may be null) is then 1 where d_min is the field's
    mpcmp_clearance check_clearance_certified_field(double margin = 0.0, int n_start = 4, int max_depth = 10, mpcmp_clearance_cert *cert = nullptr,
                                                    bool merge = false, int self_gap = 0, int *source = nullptr) {
        mpcmp_clearance r;
        mpcmp_clearance_cert c;
        chk(mpcmp_clearance_certified_field_batch(ctx_, 1, sol_x_.data(), &sol_T_, margin, n_start, max_depth, &r, &c));
        if (source) *source = 1;
        if (merge) {
            mpcmp_clearance_cert ca;
            const mpcmp_clearance a = check_clearance_certified(margin, self_gap, n_start, max_depth, &ca);
            chk(mpcmp_clearance_merge_batch(ctx_, 1, &a, &r, &r, source));
            chk(mpcmp_clearance_cert_merge_batch(ctx_, 1, &ca, &c, &c));
        }
        if (cert) *cert = c;
        return r;
    }
    // The obstacles of set_obstacles that move (include/mpcmp_moving.h): track_of [n_obs] (-1: stands still), offsets [n_tracks][n_key][3] on the
    // world clock t0 + k dt.  n_tracks == 0: the world stands still again, as it does after the next set_obstacles
    void set_moving_obstacles(int n_obs, const int *track_of, int n_tracks, int n_key, double t0, double dt, const double *offsets) {
        chk(mpcmp_set_obstacle_tracks(ctx_, 1, n_obs, track_of, n_tracks, n_key, t0, dt, offsets));
    }
    // clearance record of the last solution started at the world time t_start in the moving world, times on the running clock; retimed: on the
    // profile of the last retime() (call it first), otherwise on the plan's own clock
    mpcmp_clearance check_clearance_timed(double t_start = 0.0, int n_pts = 200, double margin = 0.0, int self_gap = 0, bool retimed = false) {
        if (retimed && retime_grid_ < 1) throw std::runtime_error("check_clearance_timed: call retime() first");
        mpcmp_clearance r;
        chk(mpcmp_clearance_timed_batch(ctx_, 1, sol_x_.data(), &sol_T_, retimed ? retime_grid_ : 0, retimed ? retime_prof_.data() : nullptr, &t_start,
                                        n_pts, margin, self_gap, &r));
        return r;
    }
    // the lowest of the K candidate start delays (ascending, >= 0) whose run has no sample under `margin`; check_wait: the wait at the start posture is
    // checked at the candidate delays too.  d_min_all [K] may be null
    mpcmp_start_delay first_clear_start(const double *delays, int K, bool check_wait = true, int n_pts = 200, double margin = 0.0, int self_gap = 0,
                                        bool retimed = false, double *d_min_all = nullptr) {
        if (retimed && retime_grid_ < 1) throw std::runtime_error("first_clear_start: call retime() first");
        mpcmp_start_delay r;
        chk(mpcmp_start_delay_batch(ctx_, 1, sol_x_.data(), &sol_T_, retimed ? retime_grid_ : 0, retimed ? retime_prof_.data() : nullptr, K, delays,
                                    check_wait ? 1 : 0, n_pts, margin, self_gap, d_min_all, &r));
        return r;
    }
    // certified clearance record of the last solution in the moving world (include/mpcmp_moving_cert.h): the motion starts at the world time t_start
    // after a wait of wait_before at the start posture and is followed by a hold of hold_after at the target; status 0 means that no clearance falls
    // below `margin` at ANY world time in [t_start - wait_before, t_start + T + hold_after].  Times are on the record clock, which starts with the
    // wait.  On the plan's own clock only: the certificate does not survive retiming.  *cert may be null
    mpcmp_clearance check_clearance_certified_timed(double t_start = 0.0, double wait_before = 0.0, double hold_after = 0.0, double margin = 0.0,
                                                    int self_gap = 0, int n_start = 4, int n_rest = 4, int max_depth = 10,
                                                    mpcmp_clearance_cert *cert = nullptr) {
        mpcmp_clearance r;
        chk(mpcmp_clearance_certified_timed_batch(ctx_, 1, sol_x_.data(), &sol_T_, &t_start, &wait_before, &hold_after, margin, self_gap, n_start,
                                                  n_rest, max_depth, &r, cert));
        return r;
    }
    // limit record of the last solution BETWEEN its nodes, at n_pts + 1 uniform samples (include/mpcmp_limits.h): excess per group under the bounds
    // the plan was solved with, and the stretch of T that makes the kinematic groups hold.  spec NULL: tol 0, no tool speed limits
    mpcmp_limits check_limits(int n_pts = 200, const mpcmp_limits_spec *spec = nullptr) {
        mpcmp_limits r;
        chk(mpcmp_limits_batch(ctx_, 1, sol_x_.data(), sol_u_.data(), &sol_T_, n_pts, spec, &r));
        return r;
    }
    // the last solution retimed along its own path (include/mpcmp_retime.h): slowed only where it leaves the limits it was solved with, at n_grid + 1
    // grid points.  spec NULL: no tool speed limits, never faster than the plan, all groups.  The profile is kept for get_retimed_trajectory;
    // status != 0 (MPCMP_RT_INFEASIBLE, MPCMP_RT_NAN): no retimed plan
    mpcmp_retime retime(int n_grid = 200, const mpcmp_retime_spec *spec = nullptr) {
        mpcmp_retime r;
        retime_prof_.assign((size_t)2 * (n_grid > 0 ? n_grid + 1 : 1), 0.0);
        retime_grid_ = 0;
        use_payload(1);
        chk(mpcmp_retime_batch(ctx_, 1, sol_x_.data(), sol_u_.data(), &sol_T_, n_grid, spec, retime_prof_.data(), &r));
        retime_grid_ = n_grid;
        return r;
    }
    // get_MPC_trajectory on the retimed clock: NP + 1 samples at uniform times in [0, T_new] (mpcmp_sample_retimed_batch); call retime() first.
    // NaN throughout if the plan could not be retimed
    template <const int NP>
    void get_retimed_trajectory(mpcmp_shim::Mat<1, NP + 1> &time, mpcmp_shim::Mat<7, NP + 1> &position_trajectory,
                                mpcmp_shim::Mat<7, NP + 1> &velocity_trajectory, mpcmp_shim::Mat<7, NP + 1> &acceleration_trajectory,
                                mpcmp_shim::Mat<7, NP + 1> &torque_trajectory) {
        if (retime_grid_ < 1) throw std::runtime_error("get_retimed_trajectory: call retime() first");
        std::vector<double> out((size_t)(NP + 1) * 29);
        use_payload(1);
        chk(mpcmp_sample_retimed_batch(ctx_, 1, sol_x_.data(), sol_u_.data(), &sol_T_, retime_grid_, retime_prof_.data(), NP, out.data()));
        unpack<NP>(out, time, position_trajectory, velocity_trajectory, acceleration_trajectory, torque_trajectory);
    }
    // limit record of the RETIMED plan between its grid points, at n_pts + 1 uniform times in [0, T_new] (include/mpcmp_retimed_check.h): the
    // record of check_limits for the motion the profile of the last retime() stands for, times on the retimed clock; call retime() first.  T_new
    // (may be NULL): the retimed duration.  status MPCMP_LIM_NAN and T_new +inf if the plan could not be retimed.  spec NULL: tol 0, no tool limits
    mpcmp_limits check_retimed_limits(int n_pts = 200, const mpcmp_limits_spec *spec = nullptr, double *T_new = nullptr) {
        if (retime_grid_ < 1) throw std::runtime_error("check_retimed_limits: call retime() first");
        mpcmp_limits r;
        use_payload(1);
        chk(mpcmp_limits_retimed_batch(ctx_, 1, sol_x_.data(), sol_u_.data(), &sol_T_, retime_grid_, retime_prof_.data(), n_pts, spec, &r, T_new));
        return r;
    }

    // A straight tool line from the current state's posture to the pose (R row-major [9], p [3]) as the plan (include/mpcmp_toolpath.h): it becomes the
    // last solution, so check_limits, check_clearance, retime, get_retimed_trajectory and get_MPC_trajectory apply to it.  T <= 0: the duration
    // from the tool-speed maxima of spec (NULL: the defaults).  status & MPCMP_TL_STOPPED: the line met a singularity or left the workspace at
    // node k_fail, and the nodes from there on are NaN
    mpcmp_tool_line plan_tool_line(const double *R, const double *p, double T = 0.0, const mpcmp_tool_line_spec *spec = nullptr) {
        mpcmp_tool_line r;
        chk(mpcmp_tool_line_batch(ctx_, 1, 0, current_state.data(), R, p, &T, spec, sol_x_.data(), sol_u_.data(), &sol_T_, &r));
        retime_grid_ = 0;
        warm_x_ = sol_x_; warm_u_ = sol_u_; warm_T_ = sol_T_; have_warm_ = true;      // (a tool line is a legal start guess of the next solve)
        for (int k = 0; k < 9; k++) line_R_[k] = R[k];
        for (int k = 0; k < 3; k++) line_p_[k] = p[k];
        have_line_ = true;
        return r;
    }
    // how far the interpolant of that plan leaves its line at n_pts + 1 uniform samples; it holds for the retimed plan as well
    mpcmp_tool_dev check_tool_line(int n_pts = 200, double tol_lin = INFINITY, double tol_ang = INFINITY) {
        if (!have_line_) throw std::runtime_error("check_tool_line: call plan_tool_line() first");
        mpcmp_tool_dev r;
        chk(mpcmp_tool_deviation_batch(ctx_, 1, 0, sol_x_.data(), line_R_, line_p_, n_pts, tol_lin, tol_ang, &r));
        return r;
    }

    // one draw in [-1,1) of the planner's seeded stream: what `Matrix<...>::Random()` coefficients are in the reference's examples
    double random_unit() { return uniform(); }
    // motionPlanner.cpp:102-114 (Eigen::Random replaced by a SplitMix64 stream owned by the planner)
    void sample_random_state(Vec7 &random_position, Vec7 &random_velocity) {
        double p7[3];
        do {
            for (int j = 0; j < 7; j++) {
                const double s = (1 - margin_position_) * (robot.max_position(j) - robot.min_position(j)) / 2;
                random_position(j) = 0.5 * (uniform() * (robot.max_position(j) - robot.min_position(j) - 2 * s) +
                                            (robot.max_position(j) + robot.min_position(j)));
            }
            robot.forward_kinematics(random_position.data(), p7, nullptr);
        } while (p7[2] < robot.min_height);
        for (int j = 0; j < 7; j++) random_velocity(j) = margin_velocity_ * uniform() * robot.max_velocity(j);
    }
    void seed(uint64_t s) { rng_ = s; }

    // motionPlanner.cpp:116-144
    int check_state_in_bounds(Vec7 &position, Vec7 &velocity, Vec7 acceleration = Vec7::Zero()) {
        bool pc = false, vc = false, ac = false;
        for (int j = 0; j < 7; j++) {
            const double s = (1 - margin_position_) * (robot.max_position(j) - robot.min_position(j)) / 2;
            pc |= position(j) > robot.max_position(j) - s || position(j) < robot.min_position(j) + s;
            vc |= std::fabs(velocity(j)) > margin_velocity_ * robot.max_velocity(j);
            ac |= std::fabs(acceleration(j)) > margin_acceleration_ * robot.max_acceleration(j);
        }
        int flag = 0;
        if (pc && !vc) flag = 1;
        if (!pc && vc) flag = 2;
        if (pc && vc) flag = 3;
        if (ac) flag += 10;
        return flag;
    }

    // motionPlanner.hpp:145-172: regularly time-spaced trajectory, nearest-sample pick round(t*(nPoint-1))
    void warm_start(double final_time, const std::vector<double> &position_trajectory /*7 x nPoint col-major*/,
                    const std::vector<double> &velocity_trajectory, const std::vector<double> &acceleration_trajectory) {
        const int nPoint = (int)(position_trajectory.size() / 7);
        std::vector<double> tau(N_);
        mpcmp_time_nodes(config.num_seg, tau.data());
        warm_x_.assign((size_t)14 * N_, 0.0); warm_u_.assign((size_t)7 * N_, 0.0);
        for (int i = 0; i < N_; i++) {
            const int idx = (int)std::lround(tau[i] * (nPoint - 1));
            for (int j = 0; j < 7; j++) {
                warm_x_[14 * i + j] = position_trajectory[7 * idx + j];
                warm_x_[14 * i + 7 + j] = velocity_trajectory[7 * idx + j];
                warm_u_[7 * i + j] = acceleration_trajectory[7 * idx + j];
            }
        }
        warm_T_ = final_time; have_warm_ = true;
    }

#if defined(MPCMP_USE_EIGEN) || (defined(__has_include) && __has_include(<Eigen/Dense>))
    // the reference's own signature (motionPlanner.hpp:145): 7 x nPoint matrices, regularly time spaced
    void warm_start(double final_time, Eigen::MatrixXd position_trajectory, Eigen::MatrixXd velocity_trajectory,
                    Eigen::MatrixXd acceleration_trajectory) {
        const size_t cnt = (size_t)position_trajectory.size();
        warm_start(final_time, std::vector<double>(position_trajectory.data(), position_trajectory.data() + cnt),
                   std::vector<double>(velocity_trajectory.data(), velocity_trajectory.data() + cnt),
                   std::vector<double>(acceleration_trajectory.data(), acceleration_trajectory.data() + cnt));
    }
#endif

    // motionPlanner.cpp:177-208.  true: jerk-limited, time-synchronised trajectory between the two states (what the
    // reference gets from Ruckig, motionPlanner.cpp:146-175); false: previous solution / warm_start() guess
    void solve_trajectory(bool use_ruckig_as_warm_start) {
        const bool use_guess = !use_ruckig_as_warm_start && have_warm_;
        if (!use_guess) {
            guess_x_.assign((size_t)14 * N_, 0.0); guess_u_.assign((size_t)7 * N_, 0.0);
            // the whole of `input`, as warm_start_RK hands it to otg.calculate (motionPlanner.cpp:146-149): states and boundary accelerations
            // (written by set_current_state / set_target_state, motionPlanner.cpp:36-38,50-52, or by the caller), velocity / acceleration / jerk limits
            // (set_constraint_margins, motionPlanner.cpp:86-88, or the caller)
            input_states(guess_x0_, guess_xf_);
            for (int j = 0; j < 7; j++) { guess_a0_[j] = input.current_acceleration[j]; guess_aT_[j] = input.target_acceleration[j]; }
            guess_in_ = input;
            chk(mpcmp_warm_start_jerk_lim_batch(ctx_, 1, guess_x0_, guess_xf_, guess_a0_, guess_aT_, input.max_velocity.data(), input.max_acceleration.data(),
                                                input.max_jerk.data(), guess_x_.data(), guess_u_.data(), &guess_T_));
            guess_is_profile_ = true;
        } else { guess_x_ = warm_x_; guess_u_ = warm_u_; guess_T_ = warm_T_; guess_is_profile_ = false; }
        solve_from_guess();
    }

    // B independent problems in one call (the loop of examples/benchmark.cpp:16). x0/xf: [B][14]
    void solve_batch(int B, const double *x0, const double *xf, double *sol_x, double *sol_u, double *sol_T, mpcmp_info *info) {
        use_payload(B);
        chk(mpcmp_solve_batch(ctx_, B, x0, xf, nullptr, nullptr, nullptr, sol_x, sol_u, sol_T, info));
    }

    // motionPlanner.hpp:99-116
    template <const int NP>
    void get_MPC_trajectory(mpcmp_shim::Mat<1, NP + 1> &time, mpcmp_shim::Mat<7, NP + 1> &position_trajectory,
                            mpcmp_shim::Mat<7, NP + 1> &velocity_trajectory, mpcmp_shim::Mat<7, NP + 1> &acceleration_trajectory,
                            mpcmp_shim::Mat<7, NP + 1> &torque_trajectory) {
        std::vector<double> out((size_t)(NP + 1) * 29);
        use_payload(1);
        chk(mpcmp_sample_batch(ctx_, 1, sol_x_.data(), sol_u_.data(), &sol_T_, NP, out.data()));
        unpack<NP>(out, time, position_trajectory, velocity_trajectory, acceleration_trajectory, torque_trajectory);
    }
    // extension beyond the reference's members: the move current_state -> vias[0] -> .. -> target_state, passed without stopping (mpcmp.h, "via-point
    // routes").  vias: M joint configurations; the velocities at the vias follow the chord rule at `speed` in [0, 1].  The legs start from the
    // jerk-limited guess with the limits of `input`.  Afterwards last_info is the record of the whole route (T = its duration), route_seam the
    // record of its junctions (accelerations are not continuous at a via), route_leg_T the legs' durations; get_route_trajectory samples it.
    mpcmp_route_seam route_seam{};
    std::vector<double> route_leg_T;
    void solve_route(const std::vector<Vec7> &vias, double speed = 0.5) {
        const int M = (int)vias.size(), L = M + 1;
        std::vector<double> via((size_t)7 * M + 1);
        for (int i = 0; i < M; i++) for (int j = 0; j < 7; j++) via[(size_t)7 * i + j] = vias[i](j);
        route_x_.assign((size_t)14 * N_ * L, 0.0); route_u_.assign((size_t)7 * N_ * L, 0.0); route_leg_T.assign(L, 0.0);
        double T = 0.0;
        route_grid_ = 0;           // (a profile belongs to the route it was computed for)
        use_payload(L);
        chk(mpcmp_solve_route_batch(ctx_, 1, M, current_state.data(), M ? via.data() : nullptr, nullptr, &speed, target_state.data(), input.max_jerk.data(),
                                    route_x_.data(), route_u_.data(), route_leg_T.data(), nullptr, &T, &last_info, &route_seam, nullptr));
    }
    // the route variant of get_MPC_trajectory: NP + 1 samples on a uniform clock across the junctions (mpcmp_sample_route_batch)
    template <const int NP>
    void get_route_trajectory(mpcmp_shim::Mat<1, NP + 1> &time, mpcmp_shim::Mat<7, NP + 1> &position_trajectory,
                              mpcmp_shim::Mat<7, NP + 1> &velocity_trajectory, mpcmp_shim::Mat<7, NP + 1> &acceleration_trajectory,
                              mpcmp_shim::Mat<7, NP + 1> &torque_trajectory) {
        if (route_leg_T.empty()) throw std::runtime_error("get_route_trajectory: no route solved yet (solve_route)");
        const int L = (int)route_leg_T.size();
        std::vector<double> out((size_t)(NP + 1) * 29);
        use_payload(L);
        chk(mpcmp_sample_route_batch(ctx_, 1, L - 1, route_x_.data(), route_u_.data(), route_leg_T.data(), NP, out.data()));
        unpack<NP>(out, time, position_trajectory, velocity_trajectory, acceleration_trajectory, torque_trajectory);
    }
    // the last route retimed as ONE path with one rate profile across its via points (include/mpcmp_route_retime.h), at n_grid + 1 grid points per
    // leg.  spec NULL: no tool speed limits, never faster than the plan, all groups.  The profile is kept for get_retimed_route_trajectory and the
    // legs' new durations in route_leg_T_new; status != 0 (MPCMP_RT_INFEASIBLE, MPCMP_RT_NAN): no retimed route
    std::vector<double> route_leg_T_new;
    mpcmp_route_retime retime_route(int n_grid = 200, const mpcmp_retime_spec *spec = nullptr) {
        if (route_leg_T.empty()) throw std::runtime_error("retime_route: no route solved yet (solve_route)");
        const int L = (int)route_leg_T.size();
        mpcmp_route_retime r;
        route_prof_.assign((size_t)2 * L * (n_grid > 0 ? n_grid + 1 : 1), 0.0);
        route_leg_T_new.assign(L, 0.0);
        route_grid_ = 0;
        use_payload(L);
        chk(mpcmp_retime_route_batch(ctx_, 1, L - 1, route_x_.data(), route_u_.data(), route_leg_T.data(), n_grid, spec, route_prof_.data(),
                                     route_leg_T_new.data(), &r));
        route_grid_ = n_grid;
        return r;
    }
    // get_route_trajectory on the retimed clock: NP + 1 samples at uniform times in [0, T_new] (mpcmp_sample_retimed_route_batch); call
    // retime_route() first.  NaN throughout if the route could not be retimed
    template <const int NP>
    void get_retimed_route_trajectory(mpcmp_shim::Mat<1, NP + 1> &time, mpcmp_shim::Mat<7, NP + 1> &position_trajectory,
                                      mpcmp_shim::Mat<7, NP + 1> &velocity_trajectory, mpcmp_shim::Mat<7, NP + 1> &acceleration_trajectory,
                                      mpcmp_shim::Mat<7, NP + 1> &torque_trajectory) {
        if (route_grid_ < 1 || route_leg_T.empty()) throw std::runtime_error("get_retimed_route_trajectory: call retime_route() first");
        const int L = (int)route_leg_T.size();
        std::vector<double> out((size_t)(NP + 1) * 29);
        use_payload(L);
        chk(mpcmp_sample_retimed_route_batch(ctx_, 1, L - 1, route_x_.data(), route_u_.data(), route_leg_T.data(), route_grid_, route_prof_.data(), NP,
                                             out.data()));
        unpack<NP>(out, time, position_trajectory, velocity_trajectory, acceleration_trajectory, torque_trajectory);
    }
    // limit record of the RETIMED route between its grid points, at n_pts + 1 uniform times of the route clock (include/mpcmp_retimed_check.h),
    // every sample under the rows of its leg; call retime_route() first.  T_new (may be NULL): the retimed duration of the route
    mpcmp_limits check_retimed_route_limits(int n_pts = 200, const mpcmp_limits_spec *spec = nullptr, double *T_new = nullptr) {
        if (route_grid_ < 1 || route_leg_T.empty()) throw std::runtime_error("check_retimed_route_limits: call retime_route() first");
        const int L = (int)route_leg_T.size();
        mpcmp_limits r;
        use_payload(L);
        chk(mpcmp_limits_retimed_route_batch(ctx_, 1, L - 1, route_x_.data(), route_u_.data(), route_leg_T.data(), route_grid_, route_prof_.data(),
                                             n_pts, spec, &r, T_new));
        return r;
    }
    // motionPlanner.hpp:73-96 — the jerk-limited trajectory of the last solve_trajectory(true) sampled uniformly, torques by
    // RNEA (motionPlanner.hpp:92); after a solve from another guess: that guess, resampled like the MPC solution
    template <const int NP>
    void get_ruckig_trajectory(mpcmp_shim::Mat<1, NP + 1> &time, mpcmp_shim::Mat<7, NP + 1> &position_trajectory,
                               mpcmp_shim::Mat<7, NP + 1> &velocity_trajectory, mpcmp_shim::Mat<7, NP + 1> &acceleration_trajectory,
                               mpcmp_shim::Mat<7, NP + 1> &torque_trajectory) {
        std::vector<double> out((size_t)(NP + 1) * 29);
        if (guess_is_profile_) {
            std::vector<double> tr((size_t)(NP + 1) * 22), q((size_t)(NP + 1) * 7), v(q.size()), a(q.size()), tau(q.size());
            chk(mpcmp_jerk_trajectory_lim_batch(ctx_, 1, guess_x0_, guess_xf_, guess_a0_, guess_aT_, guess_in_.max_velocity.data(), guess_in_.max_acceleration.data(),
                                                guess_in_.max_jerk.data(), NP, tr.data(), nullptr));
            for (int i = 0; i <= NP; i++)
                for (int j = 0; j < 7; j++) { q[(size_t)i * 7 + j] = tr[(size_t)i * 22 + 1 + j]; v[(size_t)i * 7 + j] = tr[(size_t)i * 22 + 8 + j]; a[(size_t)i * 7 + j] = tr[(size_t)i * 22 + 15 + j]; }
            use_payload(0);
            chk(mpcmp_rnea_batch(ctx_, NP + 1, q.data(), v.data(), a.data(), tau.data()));
            for (int i = 0; i <= NP; i++) {
                out[(size_t)i * 29] = tr[(size_t)i * 22];
                for (int j = 0; j < 7; j++) {
                    out[(size_t)i * 29 + 1 + j] = q[(size_t)i * 7 + j]; out[(size_t)i * 29 + 8 + j] = v[(size_t)i * 7 + j];
                    out[(size_t)i * 29 + 15 + j] = a[(size_t)i * 7 + j]; out[(size_t)i * 29 + 22 + j] = tau[(size_t)i * 7 + j];
                }
            }
        } else {
            use_payload(1);
            chk(mpcmp_sample_batch(ctx_, 1, guess_x_.data(), guess_u_.data(), &guess_T_, NP, out.data()));
        }
        unpack<NP>(out, time, position_trajectory, velocity_trajectory, acceleration_trajectory, torque_trajectory);
    }
    // motionPlanner.hpp:118-128, including its clamp: for time >= T the normalised time is set to T (not 1)
    void get_MPC_point(double time, Vec7 &position, Vec7 &velocity, Vec7 &acceleration, Vec7 &torque) {
        double o[28];
        use_payload(1);
        chk(mpcmp_mpc_point_batch(ctx_, 1, sol_x_.data(), sol_u_.data(), &sol_T_, &time, o));       // one launch: clamp, interpolation, RNEA
        for (int j = 0; j < 7; j++) { position(j) = o[j]; velocity(j) = o[7 + j]; acceleration(j) = o[14 + j]; torque(j) = o[21 + j]; }
    }
    // motionPlanner.hpp:130-142: the jerk-limited (Ruckig stand-in) trajectory of the last solve_trajectory(true) at
    // min(time, duration), torque by RNEA
    void get_RK_point(double time, Vec7 &position, Vec7 &velocity, Vec7 &acceleration, Vec7 &torque) {
        double o[28];
        chk(mpcmp_jerk_point_lim_batch(ctx_, 1, guess_x0_, guess_xf_, guess_a0_, guess_aT_, guess_in_.max_velocity.data(), guess_in_.max_acceleration.data(),
                                       guess_in_.max_jerk.data(), &time, o, nullptr));
        for (int j = 0; j < 7; j++) { position(j) = o[j]; velocity(j) = o[7 + j]; acceleration(j) = o[14 + j]; torque(j) = o[21 + j]; }
    }
    double solution_T() const { return sol_T_; }
    double guess_T() const { return guess_T_; }      // duration of the guess the last solve started from (p_guess, motionPlanner.cpp:173)
    const std::vector<double> &solution_x() const { return sol_x_; }
    const std::vector<double> &solution_u() const { return sol_u_; }
    int num_nodes() const { return N_; }
    mpcmp_ctx *context() { return ctx_; }

    // analysis/optimal_solution.txt: row 0 target, rows 1..NP+1 initial guess ("Ruckig"), then MPC; 29 columns
    // (examples/offline_trajectory.cpp:69-105)
    template <const int NP>
    void write_optimal_solution(const std::string &path) {
        mpcmp_shim::Mat<1, NP + 1> t; mpcmp_shim::Mat<7, NP + 1> q, v, a, tau;
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) throw std::runtime_error("cannot open " + path);
        std::fprintf(f, "0");
        for (int j = 0; j < 14; j++) std::fprintf(f, " %.6g", target_state(j));
        for (int j = 0; j < 14; j++) std::fprintf(f, " 0");
        std::fprintf(f, "\n");
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 0) get_ruckig_trajectory<NP>(t, q, v, a, tau); else get_MPC_trajectory<NP>(t, q, v, a, tau);
            for (int i = 0; i <= NP; i++) {
                std::fprintf(f, "%.6g", t(0, i));
                for (int j = 0; j < 7; j++) std::fprintf(f, " %.6g", q(j, i));
                for (int j = 0; j < 7; j++) std::fprintf(f, " %.6g", v(j, i));
                for (int j = 0; j < 7; j++) std::fprintf(f, " %.6g", a(j, i));
                for (int j = 0; j < 7; j++) std::fprintf(f, " %.6g", tau(j, i));
                std::fprintf(f, "\n");
            }
        }
        std::fclose(f);
    }

    // The 1000-iteration loop of examples/benchmark.cpp as ONE batched call: targets xf [B][14] from the current state,
    // then one 162-number row per problem appended to `path` in the reference's layout (benchmark.cpp:164-194):
    //   guess min(28) max(28) | MPC min(28) max(28) | guess terminal error(14) | MPC terminal error(14) |
    //   guess flags(4: jerk, linear vel, angular vel, collision) | MPC flags(4) | target(14)
    // ("guess" = the jerk-limited trajectory standing in for Ruckig, in the node form handed to the solver).
    void benchmark_batch(int B, const double *xf, const std::string &path, int n_pts = 200) {
        const size_t N = (size_t)N_;
        std::vector<double> x0((size_t)B * 14), gx(B * 14 * N), gu(B * 7 * N), gT(B), sx(B * 14 * N), su(B * 7 * N), sT(B);
        std::vector<double> sg((size_t)B * 74), sm((size_t)B * 74);
        std::vector<mpcmp_info> info(B);
        for (int b = 0; b < B; b++) for (int r = 0; r < 14; r++) x0[(size_t)b * 14 + r] = current_state(r);
        chk(mpcmp_warm_start_jerk_lim_batch(ctx_, B, x0.data(), xf, nullptr, nullptr, input.max_velocity.data(), input.max_acceleration.data(), input.max_jerk.data(),
                                            gx.data(), gu.data(), gT.data()));     // benchmark.cpp:46-47
        use_payload(B);
        chk(mpcmp_solve_batch(ctx_, B, x0.data(), xf, gx.data(), gu.data(), gT.data(), sx.data(), su.data(), sT.data(), info.data()));
        chk(mpcmp_traj_stats_batch(ctx_, B, gx.data(), gu.data(), gT.data(), xf, n_pts, sg.data()));
        chk(mpcmp_traj_stats_batch(ctx_, B, sx.data(), su.data(), sT.data(), xf, n_pts, sm.data()));
        FILE *f = std::fopen(path.c_str(), "a");
        if (!f) throw std::runtime_error("cannot open " + path);
        for (int b = 0; b < B; b++) {
            const double *g = sg.data() + (size_t)b * 74, *m = sm.data() + (size_t)b * 74;
            for (int i = 0; i < 56; i++) std::fprintf(f, "%.6g ", g[i]);
            for (int i = 0; i < 56; i++) std::fprintf(f, "%.6g ", m[i]);
            for (int i = 56; i < 70; i++) std::fprintf(f, "%.6g ", g[i]);
            for (int i = 56; i < 70; i++) std::fprintf(f, "%.6g ", m[i]);
            for (int i = 70; i < 74; i++) std::fprintf(f, "%d ", (int)g[i]);
            for (int i = 70; i < 74; i++) std::fprintf(f, "%d ", (int)m[i]);
            for (int i = 0; i < 14; i++) std::fprintf(f, i == 13 ? "%.6g\n" : "%.6g ", xf[(size_t)b * 14 + i]);
        }
        std::fclose(f);
    }

  private:
    friend struct mpcmp_shim::MpcView;
    friend struct mpcmp_shim::Trajectory;
    friend struct mpcmp_shim::Otg;
    mpcmp_ctx *ctx_ = nullptr;
    int N_ = 0, max_batch_ = 0;
    std::vector<double> sol_x_, sol_u_, warm_x_, warm_u_, guess_x_, guess_u_, route_x_, route_u_, retime_prof_, route_prof_;
    int retime_grid_ = 0;      // n_grid of the profile retime() left, 0: none
    int route_grid_ = 0;       // n_grid of the profile retime_route() left, 0: none
    double line_R_[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, line_p_[3] = {0, 0, 0};      // the goal pose of the last plan_tool_line
    bool have_line_ = false;
    double sol_T_ = 0, warm_T_ = 0, guess_T_ = 0;
    bool guess_is_profile_ = false;                 // the last guess came from the jerk-limited generator
    double guess_x0_[14] = {0}, guess_xf_[14] = {0}, guess_a0_[7] = {0}, guess_aT_[7] = {0};      // states and boundary accelerations of the last jerk-limited guess
    mpcmp_shim::InputParameter guess_in_;          // `input` as it was when that guess was made (limits of get_ruckig_trajectory / get_RK_point)
    void input_states(double *x0, double *xf) const {
        for (int j = 0; j < 7; j++) { x0[j] = input.current_position[j]; x0[7 + j] = input.current_velocity[j]; xf[j] = input.target_position[j]; xf[7 + j] = input.target_velocity[j]; }
    }
    bool have_warm_ = false;
    uint64_t rng_ = 20240001ull;
    mpcmp_payload payload_{};                       // set_payload
    bool has_payload_ = false;
    int payload_rows_ = 0;                          // rows of it the context holds now (0: none, the model's own dynamics)
    // `rows` copies of the payload into the context before a call on `rows` problems; rows = 0: the unloaded model
    void use_payload(int rows) {
        if (!has_payload_) rows = 0;
        if (rows == payload_rows_) return;
        if (rows == 0) chk(mpcmp_set_payloads(ctx_, 0, nullptr));
        else { std::vector<mpcmp_payload> t((size_t)rows, payload_); chk(mpcmp_set_payloads(ctx_, rows, t.data())); }
        payload_rows_ = rows;
    }

    // mpc.solve() from (guess_x_, guess_u_, guess_T_), then "Fix initial and final point at correct place" (motionPlanner.cpp:184-207)
    void solve_from_guess() {
        use_payload(1);
        chk(mpcmp_solve_batch(ctx_, 1, current_state.data(), target_state.data(), guess_x_.data(), guess_u_.data(), &guess_T_,
                              sol_x_.data(), sol_u_.data(), &sol_T_, &last_info));
        warm_x_ = sol_x_; warm_u_ = sol_u_; warm_T_ = sol_T_; have_warm_ = true;
        have_line_ = false;
        for (int r = 0; r < 14; r++) { warm_x_[r] = current_state(r); warm_x_[(size_t)14 * (N_ - 1) + r] = target_state(r); }
    }
    void chk(int rc) { if (rc) throw std::runtime_error(std::string("mpcmp: ") + mpcmp_last_error(ctx_)); }
    void push_config() { if (ctx_) chk(mpcmp_set_config(ctx_, &config)); }
    double uniform() {   // [-1,1), SplitMix64
        uint64_t z = (rng_ += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
    void interpolate(double t, Vec7 &q, Vec7 &v, Vec7 &a) const {   // mpc.solution_x_at / solution_u_at
        static const double xi[4] = {-1.0, -0.5, 0.5, 1.0};
        const int ns = config.num_seg;
        int s = (int)std::floor(t * ns); if (s >= ns) s = ns - 1; if (s < 0) s = 0;
        const double x = 2.0 * (t * ns - s) - 1.0;
        double L[4];
        for (int j = 0; j < 4; j++) { double w = 1; for (int k = 0; k < 4; k++) if (k != j) w *= (x - xi[k]) / (xi[j] - xi[k]); L[j] = w; }
        for (int r = 0; r < 7; r++) {
            q(r) = v(r) = a(r) = 0;
            for (int j = 0; j < 4; j++) {
                q(r) += L[j] * sol_x_[(size_t)14 * (3 * s + j) + r]; v(r) += L[j] * sol_x_[(size_t)14 * (3 * s + j) + 7 + r];
                a(r) += L[j] * sol_u_[(size_t)7 * (3 * s + j) + r];
            }
        }
    }
    template <const int NP>
    static void unpack(const std::vector<double> &out, mpcmp_shim::Mat<1, NP + 1> &time, mpcmp_shim::Mat<7, NP + 1> &q,
                       mpcmp_shim::Mat<7, NP + 1> &v, mpcmp_shim::Mat<7, NP + 1> &a, mpcmp_shim::Mat<7, NP + 1> &tau) {
        for (int i = 0; i <= NP; i++) {
            const double *o = out.data() + (size_t)i * 29;
            time(0, i) = o[0];
            for (int j = 0; j < 7; j++) { q(j, i) = o[1 + j]; v(j, i) = o[8 + j]; a(j, i) = o[15 + j]; tau(j, i) = o[22 + j]; }
        }
    }
};

// ---- MpcView members (need the complete MotionPlanner) ----
inline mpcmp_shim::MpcView::Settings mpcmp_shim::MpcView::settings() { return {owner->config.sqp_iters, owner->config.ls_iters}; }
inline mpcmp_shim::MpcView::QpSettings mpcmp_shim::MpcView::qp_settings() { return {owner->config.qp_iters, owner->config.eps_rel, owner->config.eps_abs}; }
inline std::array<double, 1> mpcmp_shim::MpcView::solution_p() const { return {owner->sol_T_}; }
inline const std::vector<double> &mpcmp_shim::MpcView::solution_x() const { return owner->sol_x_; }
inline const std::vector<double> &mpcmp_shim::MpcView::solution_u() const { return owner->sol_u_; }
inline mpcmp_shim::Mat<2 * NDOF, 1> mpcmp_shim::MpcView::solution_x_at(double t) const {
    MotionPlanner::Vec7 q, v, a; owner->interpolate(t, q, v, a);
    Mat<2 * NDOF, 1> x;
    for (int j = 0; j < 7; j++) { x(j) = q(j); x(7 + j) = v(j); }
    return x;
}
inline mpcmp_shim::Mat<NDOF, 1> mpcmp_shim::MpcView::solution_u_at(double t) const {
    MotionPlanner::Vec7 q, v, a; owner->interpolate(t, q, v, a);
    return a;
}
inline mpcmp_shim::MpcView::InfoView mpcmp_shim::MpcView::info() const {
    return {{owner->last_info.status}, owner->last_info.sqp_iters, owner->last_info.qp_iters_total};
}
inline std::vector<double> mpcmp_shim::MpcView::time_nodes() const {
    std::vector<double> t((size_t)owner->N_);
    mpcmp_time_nodes(owner->config.num_seg, t.data());
    return t;
}
// write side
inline void mpcmp_shim::MpcView::x_guess(const std::vector<double> &x) {
    if (x.size() != (size_t)14 * owner->N_) throw std::invalid_argument("mpc.x_guess: expected 14 * N entries");
    owner->warm_x_ = x; owner->have_warm_ = true;
    if (owner->warm_u_.size() != (size_t)7 * owner->N_) owner->warm_u_.assign((size_t)7 * owner->N_, 0.0);
}
inline void mpcmp_shim::MpcView::u_guess(const std::vector<double> &u) {
    if (u.size() != (size_t)7 * owner->N_) throw std::invalid_argument("mpc.u_guess: expected 7 * N entries");
    owner->warm_u_ = u;
    if (owner->warm_x_.size() != (size_t)14 * owner->N_) owner->warm_x_.assign((size_t)14 * owner->N_, 0.0);
}
inline void mpcmp_shim::MpcView::p_guess(const std::array<double, 1> &p) { owner->warm_T_ = p[0]; }
inline void mpcmp_shim::MpcView::state_bounds(const Mat<2 * NDOF, 1> &lb, const Mat<2 * NDOF, 1> &ub) {
    for (int r = 0; r < 14; r++) { owner->config.lbx[r] = lb(r); owner->config.ubx[r] = ub(r); }
    owner->push_config();
}
inline void mpcmp_shim::MpcView::control_bounds(const Mat<NDOF, 1> &lb, const Mat<NDOF, 1> &ub) {
    for (int r = 0; r < 7; r++) { owner->config.lbu[r] = lb(r); owner->config.ubu[r] = ub(r); }
    owner->push_config();
}
inline void mpcmp_shim::MpcView::parameters_bounds(const std::array<double, 1> &lb, const std::array<double, 1> &ub) {
    owner->config.lbT = lb[0]; owner->config.ubT = ub[0];
    owner->push_config();
}
inline void mpcmp_shim::MpcView::constraints_bounds(const Mat<NDOF + 1, 1> &lb, const Mat<NDOF + 1, 1> &ub) {
    for (int r = 0; r < 8; r++) { owner->config.lbg[r] = lb(r); owner->config.ubg[r] = ub(r); }
    owner->push_config();
}
inline void mpcmp_shim::MpcView::initial_state_bounds(const Mat<2 * NDOF, 1> &lb, const Mat<2 * NDOF, 1> &ub) {
    for (int r = 0; r < 14; r++) owner->current_state(r) = 0.5 * (lb(r) + ub(r));
}
inline void mpcmp_shim::MpcView::final_state_bounds(const Mat<2 * NDOF, 1> &lb, const Mat<2 * NDOF, 1> &ub) {
    double hw = 0.0;
    for (int r = 0; r < 14; r++) { owner->target_state(r) = 0.5 * (lb(r) + ub(r)); hw = std::fmax(hw, 0.5 * (ub(r) - lb(r))); }
    owner->config.eps_target = hw;
    owner->push_config();
}
inline void mpcmp_shim::MpcView::solve() {
    if (!owner->have_warm_) throw std::logic_error("mpc.solve: no guess (x_guess / u_guess / p_guess, warm_start or a previous solve)");
    owner->guess_x_ = owner->warm_x_; owner->guess_u_ = owner->warm_u_; owner->guess_T_ = owner->warm_T_; owner->guess_is_profile_ = false;
    owner->solve_from_guess();
}

// Ruckig look-alikes.  All of `input` is honoured (states, boundary accelerations, the three limit vectors); the limits travel as arguments
// (mpcmp_jerk_point_lim_batch), the planner's configuration is neither read nor touched.
inline mpcmp_shim::Result mpcmp_shim::Otg::calculate(const InputParameter &input, Trajectory &trajectory) {
    trajectory.owner = owner; trajectory.in = input;
    trajectory.duration = -1.0;
    double x0[14], xf[14], o[28], T = 0.0, t0 = 0.0;
    for (int j = 0; j < 7; j++) { x0[j] = input.current_position[j]; x0[7 + j] = input.current_velocity[j]; xf[j] = input.target_position[j]; xf[7 + j] = input.target_velocity[j]; }
    // a failure (e.g. a limit that is not positive: ruckig::Result::ErrorInvalidInput) is the return value, not an exception
    const int rc = mpcmp_jerk_point_lim_batch(owner->ctx_, 1, x0, xf, input.current_acceleration.data(), input.target_acceleration.data(), input.max_velocity.data(),
                                              input.max_acceleration.data(), input.max_jerk.data(), &t0, o, &T);
    if (rc != MPCMP_OK || !(T >= 0.0)) return Error;
    trajectory.duration = T;
    return Working;                                         // ruckig's offline calculate() returns Working on success
}
inline void mpcmp_shim::Trajectory::at_time(double time, std::array<double, NDOF> &position, std::array<double, NDOF> &velocity,
                                            std::array<double, NDOF> &acceleration) const {
    if (!owner || duration < 0.0) throw std::logic_error("Trajectory::at_time without a successful otg.calculate");
    double x0[14], xf[14], o[28], T = 0.0;
    for (int j = 0; j < 7; j++) { x0[j] = in.current_position[j]; x0[7 + j] = in.current_velocity[j]; xf[j] = in.target_position[j]; xf[7 + j] = in.target_velocity[j]; }
    owner->chk(mpcmp_jerk_point_lim_batch(owner->ctx_, 1, x0, xf, in.current_acceleration.data(), in.target_acceleration.data(), in.max_velocity.data(),
                                          in.max_acceleration.data(), in.max_jerk.data(), &time, o, &T));
    for (int j = 0; j < 7; j++) { position[j] = o[j]; velocity[j] = o[7 + j]; acceleration[j] = o[14 + j]; }
}
