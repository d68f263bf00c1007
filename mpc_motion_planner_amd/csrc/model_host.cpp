// model_host.cpp — the host-only part of the C ABI (include/mpcmp.h): the default model, limits and configuration, the URDF reader, the rules a
// configuration, a bound row and a payload must satisfy, the single-problem kinematics of the reference's robot wrapper and the single-problem
// statements of the tool-line moves (toolpath.hpp), of the certified clearance check (clearance_cert.hpp), of the checks in a moving world
// (moving_rule.hpp), of the certified check in a moving world (moving_cert_rule.hpp) and of the voxel worlds (field_rule.hpp, frame_rule.hpp).  Plain C++: no HIP
// header is read and nothing here runs on or talks to a device, so this file can also be compiled on its own and checked with the host sanitizers
// (examples/urdf_selftest.cpp).
#include <array>
#include <cctype>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/mpcmp.h"
#include "model_host.hpp"
#include "kinematics_host.hpp"
#include "payload.hpp"
#include "plan_interp.hpp"
#include "toolpath.hpp"
#include "clearance_cert.hpp"
#include "moving_rule.hpp"
#include "moving_cert_rule.hpp"
#include "field_rule.hpp"
#include "field_cert_rule.hpp"
#include "frame_rule.hpp"

using namespace mpcmp;

thread_local std::string mpcmp::g_err;

// ------------------------------------------------------------------------------------------------
// configuration helpers (host only)
extern "C" const char *mpcmp_version(void) { return "mpcmp 0.1 (gfx950)"; }

extern "C" int mpcmp_num_nodes(int num_seg) { return 3 * num_seg + 1; }

extern "C" int mpcmp_time_nodes(int num_seg, double *tau) {
    if (num_seg < 1 || !tau) return MPCMP_EINVAL;
    for (int k = 0; k <= 3 * num_seg; k++) tau[k] = mpcmp_plan::node_time(num_seg, k);
    return MPCMP_OK;
}

extern "C" int mpcmp_default_limits(double *qmin, double *qmax, double *vmax, double *amax, double *jmax,
                                    double *taumax) {
    // Franka Emika limits as tabulated by the reference, robot_utils/pandaWrapper.hpp:29-34
    static const double t[6][7] = {{-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973},
                                   {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973},
                                   {2.1750, 2.1750, 2.1750, 2.1750, 2.6100, 2.6100, 2.6100},
                                   {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0},
                                   {7500, 3750, 5000, 6250, 7500, 10000, 10000},
                                   {87, 87, 87, 87, 12, 12, 12}};
    double *o[6] = {qmin, qmax, vmax, amax, jmax, taumax};
    for (int k = 0; k < 6; k++)
        if (o[k]) std::memcpy(o[k], t[k], sizeof t[k]);
    return MPCMP_OK;
}

extern "C" int mpcmp_set_min_height(mpcmp_config *c, double min_height) {
    if (!c) return MPCMP_EINVAL;
    c->lbg[7] = min_height;
    c->ubg[7] = INFINITY;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_margins(mpcmp_config *c, double mp, double mv, double ma, double mt) {
    if (!c) return MPCMP_EINVAL;
    double qmin[7], qmax[7], vmax[7], amax[7], tmax[7];
    mpcmp_default_limits(qmin, qmax, vmax, amax, nullptr, tmax);
    for (int j = 0; j < 7; j++) {
        const double s = (1.0 - mp) * (qmax[j] - qmin[j]) / 2.0;   // motionPlanner.cpp:66
        c->lbx[j] = qmin[j] + s; c->ubx[j] = qmax[j] - s;
        c->lbx[7 + j] = -mv * vmax[j]; c->ubx[7 + j] = mv * vmax[j];
        c->lbu[j] = -ma * amax[j]; c->ubu[j] = ma * amax[j];
        c->lbg[j] = -mt * tmax[j]; c->ubg[j] = mt * tmax[j];
    }
    c->lbT = 0.0; c->ubT = 10.0;                                  // motionPlanner.cpp:77-78
    return mpcmp_set_min_height(c, 0.05);                         // pandaWrapper.hpp:40
}

extern "C" int mpcmp_default_config(mpcmp_config *c, int num_seg, int sqp_iters) {
    if (!c || num_seg < 1) return MPCMP_EINVAL;
    std::memset(c, 0, sizeof *c);
    c->num_seg = num_seg; c->sqp_iters = sqp_iters;
    c->qp_iters = 700; c->ls_iters = 10; c->check_every = 25; c->quirk_dtau_dT = 1;
    c->eps_abs = 1e-3; c->eps_rel = 1e-3;
    c->rho = 0.02; c->sigma = 1e-6; c->alpha = 1.4; c->rho_eq_scale = 1e3;      // fitted to the reference's stored solve: tools/polympc_param_fit.py
    c->ls_eta = 0.25; c->ls_tau = 0.5; c->hess_reg = 1e-3; c->eps_target = 1e-2;
    return mpcmp_set_margins(c, 1.0, 1.0, 1.0, 1.0);              // motionPlanner.cpp:24
}

// per-problem bounds: a row is the six tables of the configuration, which lie there in the row's order without a gap
static_assert(sizeof(mpcmp_bounds) == 58 * sizeof(double), "mpcmp_bounds: 58 doubles");
static_assert(offsetof(mpcmp_config, ubg) + sizeof(double[8]) - offsetof(mpcmp_config, lbx) == sizeof(mpcmp_bounds) &&
              offsetof(mpcmp_config, ubx) - offsetof(mpcmp_config, lbx) == offsetof(mpcmp_bounds, ubx) &&
              offsetof(mpcmp_config, lbu) - offsetof(mpcmp_config, lbx) == offsetof(mpcmp_bounds, lbu) &&
              offsetof(mpcmp_config, ubu) - offsetof(mpcmp_config, lbx) == offsetof(mpcmp_bounds, ubu) &&
              offsetof(mpcmp_config, lbg) - offsetof(mpcmp_config, lbx) == offsetof(mpcmp_bounds, lbg) &&
              offsetof(mpcmp_config, ubg) - offsetof(mpcmp_config, lbx) == offsetof(mpcmp_bounds, ubg),
              "mpcmp_bounds has the layout of the six tables of mpcmp_config");
extern "C" int mpcmp_bounds_from_config(const mpcmp_config *c, mpcmp_bounds *out) {
    if (!c || !out) return MPCMP_EINVAL;
    std::memcpy(out, c->lbx, sizeof *out);
    return MPCMP_OK;
}

extern "C" int mpcmp_bounds_from_margins(double mp, double mv, double ma, double mt, double min_height, mpcmp_bounds *out) {
    if (!out) return MPCMP_EINVAL;
    mpcmp_config c;
    if (int rc = mpcmp_default_config(&c, 4, 1)) return rc;      // (the tables do not depend on num_seg or sqp_iters)
    if (int rc = mpcmp_set_margins(&c, mp, mv, ma, mt)) return rc;
    if (int rc = mpcmp_set_min_height(&c, min_height)) return rc;
    return mpcmp_bounds_from_config(&c, out);
}

static void rpy_to_R(const double rpy[3], double R[9]) {
    const double cr = std::cos(rpy[0]), sr = std::sin(rpy[0]), cp = std::cos(rpy[1]), sp = std::sin(rpy[1]),
                 cy = std::cos(rpy[2]), sy = std::sin(rpy[2]);
    // R = Rz(yaw) Ry(pitch) Rx(roll)
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

// ---- scenario helpers (host): robot_utils/pandaWrapper.cpp:14-107 ----
extern "C" int mpcmp_tool_jacobian(const mpcmp_model *model, const double *q, double *J, double *p, double *R) {
    if (!model || !q || !J) return MPCMP_EINVAL;
    double pp[3], RR[9];
    mpcmp_host::tool_jacobian(*model, q, J, pp, RR);
    if (p) for (int k = 0; k < 3; k++) p[k] = pp[k];
    if (R) for (int k = 0; k < 9; k++) R[k] = RR[k];
    return MPCMP_OK;
}

extern "C" int mpcmp_forward_velocities(const mpcmp_model *model, const double *q, const double *qd, double *out) {
    if (!model || !q || !qd || !out) return MPCMP_EINVAL;
    double J[42], p[3], R[9];
    mpcmp_host::tool_jacobian(*model, q, J, p, R);
    for (int r = 0; r < 6; r++) { double s = 0; for (int k = 0; k < 7; k++) s += J[r * 7 + k] * qd[k]; out[r] = s; }
    return MPCMP_OK;
}

extern "C" int mpcmp_inverse_velocities(const mpcmp_model *model, const double *q, const double *lin, const double *ang, double *qd) {
    if (!model || !q || !lin || !ang || !qd) return MPCMP_EINVAL;
    const double b[6] = {lin[0], lin[1], lin[2], ang[0], ang[1], ang[2]};
    return mpcmp_host::inverse_velocities(*model, q, b, qd) ? MPCMP_OK : MPCMP_ERUNTIME;
}

// the loop of PandaWrapper::inverse_kinematic around the DLS step the batched kernel shares (kinematics_host.hpp)
extern "C" int mpcmp_inverse_kinematics(const mpcmp_model *model, const double *Rdes, const double *pdes, const double *q_init,
                                        double *q, int *iters) {
    if (!model || !Rdes || !pdes || !q) return MPCMP_EINVAL;
    for (int k = 0; k < 7; k++) q[k] = q_init ? q_init[k] : 0.0;
    for (int it = 0;; it++) {
        double en;
        const int r = mpcmp_host::ik_dls_step(*model, Rdes, pdes, q, it, &en);
        if (iters) *iters = it;
        if (r == mpcmp_host::IK_CONVERGED) return MPCMP_OK;
        if (r == mpcmp_host::IK_CAPPED) return 1;
        if (r == mpcmp_host::IK_NOT_PD) return MPCMP_ERUNTIME;
    }
}

extern "C" int mpcmp_default_model(mpcmp_model *m) {
    if (!m) return MPCMP_EINVAL;
    // Kinematic / inertial parameters of the Panda arm (robot_utils/panda-model/panda_arm.urdf)
    static const double rpy[7][3] = {{0, 0, 0}, {-1.57079632679, 0, 0}, {1.57079632679, 0, 0}, {1.57079632679, 0, 0},
                                     {-1.57079632679, 0, 0}, {1.57079632679, 0, 0}, {1.57079632679, 0, 0}};
    static const double xyz[7][3] = {{0, 0, 0.333}, {0, 0, 0}, {0, -0.316, 0}, {0.0825, 0, 0},
                                     {-0.0825, 0.384, 0}, {0, 0, 0}, {0.088, 0, 0}};
    static const double mass[7] = {4.970684, 0.646926, 3.228604, 3.587895, 1.225946, 1.666555, 0.735522};
    static const double com[7][3] = {{3.875e-03, 2.081e-03, -0.1750}, {-3.141e-03, -2.872e-02, 3.495e-03},
                                     {2.7518e-02, 3.9252e-02, -6.6502e-02}, {-5.317e-02, 1.04419e-01, 2.7454e-02},
                                     {-1.1953e-02, 4.1065e-02, -3.8437e-02}, {6.0149e-02, -1.4117e-02, -1.0517e-02},
                                     {1.0517e-02, -4.252e-03, 6.1597e-02}};
    static const double in6[7][6] = {{7.0337e-01, -1.3900e-04, 6.7720e-03, 7.0661e-01, 1.9169e-02, 9.1170e-03},
                                     {7.9620e-03, -3.9250e-03, 1.0254e-02, 2.8110e-02, 7.0400e-04, 2.5995e-02},
                                     {3.7242e-02, -4.7610e-03, -1.1396e-02, 3.6155e-02, -1.2805e-02, 1.0830e-02},
                                     {2.5853e-02, 7.7960e-03, -1.3320e-03, 1.9552e-02, 8.6410e-03, 2.8323e-02},
                                     {3.5549e-02, -2.1170e-03, -4.0370e-03, 2.9474e-02, 2.2900e-04, 8.6270e-03},
                                     {1.9640e-03, 1.0900e-04, -1.1580e-03, 4.3540e-03, 3.4100e-04, 5.4330e-03},
                                     {1.2516e-02, -4.2800e-04, -1.1960e-03, 1.0027e-02, -7.4100e-04, 4.8150e-03}};
    std::memset(m, 0, sizeof *m);
    for (int i = 0; i < 7; i++) {
        rpy_to_R(rpy[i], m->R0[i]);
        std::memcpy(m->p[i], xyz[i], sizeof xyz[i]);
        m->mass[i] = mass[i];
        std::memcpy(m->com[i], com[i], sizeof com[i]);
        const double *I = in6[i];
        const double F[9] = {I[0], I[1], I[2], I[1], I[3], I[4], I[2], I[4], I[5]};
        std::memcpy(m->I[i], F, sizeof F);
    }
    m->link8[2] = 0.107;
    m->tool[2] = 0.107 + 0.15;
    m->gravity[2] = -9.81;
    // fixed children of link7: link8 (m=0, I=1e-3 Id) and panda_tool (m=1, I=1e-3 Id) are lumped into body 7
    const double mk[3] = {mass[6], 0.0, 1.0};
    const double ck[3][3] = {{com[6][0], com[6][1], com[6][2]}, {0, 0, 0.107}, {0, 0, 0.257}};
    double Ik[3][9];
    std::memcpy(Ik[0], m->I[6], sizeof Ik[0]);
    for (int k = 1; k < 3; k++) { std::memset(Ik[k], 0, sizeof Ik[k]); Ik[k][0] = Ik[k][4] = Ik[k][8] = 1e-3; }
    lump_last_body(m, 3, mk, ck, Ik);
    return MPCMP_OK;
}

// ---- URDF reader: any number of serial 7-joint chains on one base (robot_utils/pandaWrapper.cpp:3-12 takes any URDF) --------
// What the kernels need of a robot is, per chain, seven revolute joints about the z axis of their own frame, the placement of
// each joint in its parent joint's frame, one rigid body per joint frame and the two named frames behind the last joint.  A URDF
// is brought into that form here: fixed joints (before, between and behind the revolute joints, rotated or not) are folded into
// the next joint's placement and their links lumped into the body of the joint frame they hang on; a chain's base placement is
// folded into its first joint; rotated inertial frames rotate the inertia tensor; a joint axis other than +z is absorbed by a
// constant rotation of the child frame.
namespace {
struct UrdfLink { double mass = 0, com[3] = {0, 0, 0}, I[9] = {0}, irpy[3] = {0, 0, 0}; bool has_inertial = false; };
struct UrdfJoint { std::string name, type, parent, child; double xyz[3] = {0, 0, 0}, rpy[3] = {0, 0, 0}, axis[3] = {0, 0, 1}; };
struct Xf { double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}; };       // rigid transform, parent <- child

static std::string attr(const std::string &tag, const std::string &key) {
    size_t p = 0;
    while ((p = tag.find(key + "=", p)) != std::string::npos) {
        if (p > 0 && (isalnum((unsigned char)tag[p - 1]) || tag[p - 1] == '_')) { p += key.size(); continue; }
        const size_t q0 = p + key.size() + 1;
        const char quote = tag[q0];
        const size_t q1 = tag.find(quote, q0 + 1);
        return tag.substr(q0 + 1, q1 - q0 - 1);
    }
    return "";
}
static void parse3(const std::string &s, double *o) {
    if (s.empty()) return;
    std::istringstream is(s);
    is >> o[0] >> o[1] >> o[2];
}
static bool is_identity(const double *R) {
    return R[0] == 1 && R[4] == 1 && R[8] == 1 && R[1] == 0 && R[2] == 0 && R[3] == 0 && R[5] == 0 && R[6] == 0 && R[7] == 0;
}
static void matmul3(const double *A, const double *B, double *Cm) {
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Cm[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
// (identity factors are skipped, so that a URDF without rotated fixed joints gives bit-for-bit the numbers it holds)
static Xf compose(const Xf &a, const Xf &b) {
    Xf o;
    if (is_identity(a.R)) { std::memcpy(o.R, b.R, sizeof o.R); for (int d = 0; d < 3; d++) o.t[d] = a.t[d] + b.t[d]; }
    else {
        if (is_identity(b.R)) std::memcpy(o.R, a.R, sizeof o.R); else matmul3(a.R, b.R, o.R);
        for (int d = 0; d < 3; d++) o.t[d] = a.t[d] + (a.R[3 * d] * b.t[0] + a.R[3 * d + 1] * b.t[1] + a.R[3 * d + 2] * b.t[2]);
    }
    return o;
}
static void rotate_inertia(const double *R, const double *I, double *o) {          // R I R^T
    if (is_identity(R)) { std::memcpy(o, I, 9 * sizeof(double)); return; }
    double RI[9], Rt[9];
    matmul3(R, I, RI);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rt[3 * r + c] = R[3 * c + r];
    matmul3(RI, Rt, o);
}
// rotation that takes +z to the (normalised) axis a
static bool axis_rotation(const double *a_in, double *R) {
    const double n = std::sqrt(a_in[0] * a_in[0] + a_in[1] * a_in[1] + a_in[2] * a_in[2]);
    if (!(n > 0)) return false;
    const double a[3] = {a_in[0] / n, a_in[1] / n, a_in[2] / n};
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (a[0] == 0 && a[1] == 0 && a[2] == 1) { std::memcpy(R, I3, sizeof I3); return true; }
    if (a[0] == 0 && a[1] == 0 && a[2] == -1) { const double F[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1}; std::memcpy(R, F, sizeof F); return true; }
    // Rodrigues: axis v = z x a, sin = |v|, cos = a_z
    const double v[3] = {-a[1], a[0], 0.0}, c = a[2], k = 1.0 / (1.0 + c);
    const double V[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
    double V2[9];
    matmul3(V, V, V2);
    for (int i = 0; i < 9; i++) R[i] = I3[i] + V[i] + k * V2[i];
    return true;
}
struct BodyAcc { std::vector<double> m; std::vector<std::array<double, 3>> c; std::vector<std::array<double, 9>> I; };
struct ChainAcc {
    std::string first_joint;
    std::vector<Xf> placement;                      // joint i in joint i - 1 (the first: in the base / world frame)
    std::vector<BodyAcc> bodies;                    // per joint frame
    std::vector<std::vector<std::array<double, 3>>> frames;     // fixed descendants of each joint frame (origins, in order of discovery)
};
// same arithmetic, in the same order, as lump_last_body for three bodies
static void lump(const BodyAcc &b, double &M, double *c, double *It) {
    const size_t n = b.m.size();
    M = b.m[0];
    for (size_t k = 1; k < n; k++) M = M + b.m[k];
    c[0] = c[1] = c[2] = 0;
    for (size_t k = 0; k < n; k++) for (int d = 0; d < 3; d++) c[d] += b.m[k] * b.c[k][d];
    for (int d = 0; d < 3; d++) c[d] /= M;
    for (int i = 0; i < 9; i++) It[i] = 0;
    for (size_t k = 0; k < n; k++) {
        const double d[3] = {b.c[k][0] - c[0], b.c[k][1] - c[1], b.c[k][2] - c[2]};
        const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (int r = 0; r < 3; r++) for (int s2 = 0; s2 < 3; s2++)
            It[3 * r + s2] += b.I[k][3 * r + s2] + b.m[k] * ((r == s2 ? d2 : 0.0) - d[r] * d[s2]);
    }
}
}  // namespace

extern "C" int mpcmp_models_from_urdf(const char *path, int max_chains, mpcmp_model *models, int *n_chains) {
    if (!path || !models || !n_chains || max_chains < 1) return MPCMP_EINVAL;
    *n_chains = 0;
    std::ifstream f(path);
    if (!f) { g_err = std::string("cannot open URDF ") + path; return MPCMP_EINVAL; }
    std::stringstream ss; ss << f.rdbuf();
    const std::string xml = ss.str();
    std::map<std::string, UrdfLink> links;
    std::vector<std::string> link_order;
    std::vector<UrdfJoint> joints;
    size_t pos = 0;
    std::string cur_link; UrdfJoint cur_joint; bool in_link = false, in_joint = false, in_inertial = false;
    while ((pos = xml.find('<', pos)) != std::string::npos) {
        if (xml.compare(pos, 4, "<!--") == 0) { const size_t e = xml.find("-->", pos); if (e == std::string::npos) break; pos = e + 3; continue; }
        const size_t end = xml.find('>', pos);
        if (end == std::string::npos) break;
        const std::string tag = xml.substr(pos + 1, end - pos - 1);
        pos = end + 1;
        if (tag.empty() || tag[0] == '?' || tag[0] == '!') continue;
        std::istringstream ts(tag); std::string name; ts >> name;
        if (!name.empty() && name.back() == '/') name.pop_back();
        if (name == "link") { cur_link = attr(tag, "name"); if (!links.count(cur_link)) link_order.push_back(cur_link); links[cur_link]; in_link = tag.back() != '/'; }
        else if (name == "/link") in_link = false;
        else if (name == "joint" && tag.find("type=") != std::string::npos) {
            cur_joint = UrdfJoint(); cur_joint.type = attr(tag, "type"); cur_joint.name = attr(tag, "name"); in_joint = true;
        } else if (name == "/joint") { if (in_joint) joints.push_back(cur_joint); in_joint = false; }
        else if (name == "inertial") in_inertial = true;
        else if (name == "/inertial") in_inertial = false;
        else if (name == "origin") {
            if (in_joint) { parse3(attr(tag, "xyz"), cur_joint.xyz); parse3(attr(tag, "rpy"), cur_joint.rpy); }
            else if (in_link && in_inertial) { parse3(attr(tag, "xyz"), links[cur_link].com); parse3(attr(tag, "rpy"), links[cur_link].irpy); }
        } else if (name == "mass" && in_link && in_inertial) { links[cur_link].mass = atof(attr(tag, "value").c_str()); links[cur_link].has_inertial = true; }
        else if (name == "inertia" && in_link && in_inertial) {
            UrdfLink &L = links[cur_link];
            const double xx = atof(attr(tag, "ixx").c_str()), xy = atof(attr(tag, "ixy").c_str()), xz = atof(attr(tag, "ixz").c_str()),
                         yy = atof(attr(tag, "iyy").c_str()), yz = atof(attr(tag, "iyz").c_str()), zz = atof(attr(tag, "izz").c_str());
            const double F[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
            std::memcpy(L.I, F, sizeof F);
        } else if (name == "parent" && in_joint) cur_joint.parent = attr(tag, "link");
        else if (name == "child" && in_joint) cur_joint.child = attr(tag, "link");
        else if (name == "axis" && in_joint) parse3(attr(tag, "xyz"), cur_joint.axis);
    }
    if (links.empty()) { g_err = "URDF holds no links"; return MPCMP_EINVAL; }
    // the kinematic tree
    std::map<std::string, std::vector<const UrdfJoint *>> kids;
    std::map<std::string, int> is_child;
    for (auto &j : joints) {
        if (!links.count(j.parent) || !links.count(j.child)) { g_err = "joint " + j.name + " names an unknown link"; return MPCMP_EINVAL; }
        kids[j.parent].push_back(&j);
        if (is_child[j.child]++) { g_err = "link " + j.child + " has two parent joints"; return MPCMP_EINVAL; }
    }
    std::string root;
    for (auto &ln : link_order) if (!is_child.count(ln)) { if (!root.empty()) { g_err = "URDF has more than one root link"; return MPCMP_EINVAL; } root = ln; }
    if (root.empty()) { g_err = "URDF has no root link (cycle)"; return MPCMP_EINVAL; }
    std::vector<ChainAcc> chains;
    std::string err;
    // depth first in file order; C: link frame in the current model frame (the world before a chain starts, then the joint frame)
    std::function<bool(const std::string &, const Xf &, int, int)> visit = [&](const std::string &ln, const Xf &C, int ci, int ji) -> bool {
        const UrdfLink &L = links[ln];
        if (ci >= 0) {
            ChainAcc &ch = chains[ci];
            if (L.has_inertial) {
                double Rin[9], Il[9], If[9];
                rpy_to_R(L.irpy, Rin);
                rotate_inertia(Rin, L.I, Il);          // inertial frame -> link axes
                rotate_inertia(C.R, Il, If);           // link axes -> joint frame axes
                Xf com; std::memcpy(com.t, L.com, sizeof L.com);
                const Xf cj = compose(C, com);
                ch.bodies[ji].m.push_back(L.mass);
                ch.bodies[ji].c.push_back({cj.t[0], cj.t[1], cj.t[2]});
                std::array<double, 9> Ia; std::memcpy(Ia.data(), If, sizeof If);
                ch.bodies[ji].I.push_back(Ia);
            }
        }
        int revolute_kids = 0;
        for (const UrdfJoint *j : kids[ln]) {
            Xf T; rpy_to_R(j->rpy, T.R); std::memcpy(T.t, j->xyz, sizeof j->xyz);
            if (j->type == "fixed") {
                const Xf Cc = compose(C, T);
                if (ci >= 0) chains[ci].frames[ji].push_back({Cc.t[0], Cc.t[1], Cc.t[2]});
                if (!visit(j->child, Cc, ci, ji)) return false;
            } else if (j->type == "revolute" || j->type == "continuous") {
                if (ci >= 0 && ++revolute_kids > 1) { err = "link " + ln + " carries two revolute joints: not a serial chain"; return false; }
                Xf Ra;
                if (!axis_rotation(j->axis, Ra.R)) { err = "joint " + j->name + " has a zero axis"; return false; }
                int c2 = ci;
                if (c2 < 0) { chains.emplace_back(); c2 = (int)chains.size() - 1; chains[c2].first_joint = j->name; }
                else if (ji != (int)chains[c2].placement.size() - 1) { err = "joint " + j->name + " branches off the chain starting at " + chains[c2].first_joint; return false; }
                ChainAcc &ch = chains[c2];
                ch.placement.push_back(compose(compose(C, T), Ra));
                ch.bodies.emplace_back(); ch.frames.emplace_back();
                Xf Cn;                                  // child link frame in the new joint frame: the inverse of the axis rotation
                for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Cn.R[3 * r + c] = Ra.R[3 * c + r];
                if (!visit(j->child, Cn, c2, (int)ch.placement.size() - 1)) return false;
            } else { err = "joint " + j->name + ": type '" + j->type + "' is not supported (fixed, revolute, continuous)"; return false; }
        }
        return true;
    };
    // (a chain must run through consecutive joint frames: the recursion above passes the frame index down, so a revolute joint
    //  found below joint frame ji of chain ci extends that chain only if ji is its last frame)
    if (!visit(root, Xf(), -1, -1)) { g_err = err; return MPCMP_EINVAL; }
    if (chains.empty()) { g_err = "URDF holds no revolute joint"; return MPCMP_EINVAL; }
    if ((int)chains.size() > max_chains) { g_err = "URDF holds more chains than the caller has room for"; return MPCMP_ETOOBIG; }
    for (size_t ci = 0; ci < chains.size(); ci++) {
        const ChainAcc &ch = chains[ci];
        if (ch.placement.size() != 7) {
            g_err = "the chain starting at joint " + ch.first_joint + " has " + std::to_string(ch.placement.size()) + " revolute joints; the kernels are built for 7";
            return MPCMP_EINVAL;
        }
        mpcmp_model *m = models + ci;
        std::memset(m, 0, sizeof *m);
        for (int i = 0; i < 7; i++) {
            std::memcpy(m->R0[i], ch.placement[i].R, sizeof m->R0[i]);
            std::memcpy(m->p[i], ch.placement[i].t, sizeof m->p[i]);
            const BodyAcc &b = ch.bodies[i];
            if (b.m.empty()) continue;                                   // (a massless joint frame)
            if (b.m.size() == 1) { m->mass[i] = b.m[0]; std::memcpy(m->com[i], b.c[0].data(), sizeof m->com[i]); std::memcpy(m->I[i], b.I[0].data(), sizeof m->I[i]); }
            else lump(b, m->mass[i], m->com[i], m->I[i]);
        }
        // the two named frames of the reference behind the last joint (panda_link8, panda_tool: panda_arm.urdf:134-153): the first
        // and the last fixed descendant of joint frame 7
        const auto &fr = ch.frames[6];
        if (!fr.empty()) { std::memcpy(m->link8, fr.front().data(), sizeof m->link8); std::memcpy(m->tool, fr.back().data(), sizeof m->tool); }
        m->gravity[2] = -9.81;
    }
    *n_chains = (int)chains.size();
    return MPCMP_OK;
}

extern "C" int mpcmp_model_from_urdf(const char *path, mpcmp_model *m) {
    if (!path || !m) return MPCMP_EINVAL;
    mpcmp_model tmp[8];
    int n = 0;
    const int rc = mpcmp_models_from_urdf(path, 8, tmp, &n);
    if (rc != MPCMP_OK) return rc;
    if (n != 1) { g_err = "URDF holds " + std::to_string(n) + " chains: use mpcmp_models_from_urdf / mpcmp_create_multi"; return MPCMP_EINVAL; }
    *m = tmp[0];
    return MPCMP_OK;
}

// the rule of the six bound tables (of the configuration, and of every row of mpcmp_set_bounds): infinite ends are allowed (a row or box switched
// off); NaN, lb > ub and an empty box (lb = +inf or ub = -inf) are not.  A general row narrower than 1e-4 takes rho_eq (oracle/ocp.c: u - l < 1e-4);
// the assembly of k_qp and k_qp2 (num_seg 1, 2, 4) gives every general row the plain rho, so its factor would not be the matrix its iteration uses:
// such rows are supported from num_seg 6 on (k_qp3, k_qp5)
int mpcmp::validate_boxes(const mpcmp_bounds *t, std::string &err) {
    auto box_ok = [](double lb, double ub) { return lb <= ub && lb < INFINITY && ub > -INFINITY; };
    for (int i = 0; i < 14; i++) if (!box_ok(t->lbx[i], t->ubx[i])) { err = "lbx[" + std::to_string(i) + "] <= ubx[" + std::to_string(i) + "] required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    for (int i = 0; i < 7; i++) if (!box_ok(t->lbu[i], t->ubu[i])) { err = "lbu[" + std::to_string(i) + "] <= ubu[" + std::to_string(i) + "] required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    for (int i = 0; i < 8; i++) if (!box_ok(t->lbg[i], t->ubg[i])) { err = "lbg[" + std::to_string(i) + "] <= ubg[" + std::to_string(i) + "] required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}
int mpcmp::validate_general_rows(const mpcmp_bounds *t, int num_seg, std::string &err) {
    if (num_seg <= 4)
        for (int i = 0; i < 8; i++)
            if (t->ubg[i] - t->lbg[i] < 1e-4) { err = "num_seg 1, 2 and 4: ubg[" + std::to_string(i) + "] - lbg[" + std::to_string(i) + "] must be >= 1e-4 (narrower general rows need num_seg 6 or 8)"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

int mpcmp::validate(const mpcmp_config *c, std::string &err) {
    if (c->num_seg != 1 && c->num_seg != 2 && c->num_seg != 4 && c->num_seg != 6 && c->num_seg != 8) { err = "num_seg must be 1, 2, 4, 6 or 8 on the HIP backend"; return MPCMP_EINVAL; }
    if (c->sqp_iters < 1 || c->qp_iters < 1 || c->check_every < 1) { err = "iteration counts must be >= 1"; return MPCMP_EINVAL; }
    if (c->ls_iters < 2 || c->ls_iters > 10) { err = "ls_iters must be in [2,10]"; return MPCMP_EINVAL; }
    if (!(c->rho > 0) || !(c->sigma > 0) || !(c->alpha > 0 && c->alpha < 2)) { err = "rho, sigma > 0 and 0 < alpha < 2 required"; return MPCMP_EINVAL; }
    if (c->qp_warm_start < -1 || c->qp_warm_start > 1 || c->carry_multipliers < -1 || c->carry_multipliers > 1) { err = "qp_warm_start and carry_multipliers are -1, 0 or 1"; return MPCMP_EINVAL; }
    // (written as !(x >= 0) and the like, so that a NaN fails every test)
    if (!(c->eps_abs >= 0) || !(c->eps_rel >= 0) || !(c->eps_target >= 0) || !(c->hess_reg >= 0)) { err = "eps_abs, eps_rel, eps_target and hess_reg must be >= 0"; return MPCMP_EINVAL; }
    if (!(c->rho_eq_scale > 0)) { err = "rho_eq_scale must be > 0"; return MPCMP_EINVAL; }
    if (!(c->ls_eta > 0 && c->ls_eta < 1) || !(c->ls_tau > 0 && c->ls_tau < 1)) { err = "ls_eta and ls_tau must lie in (0, 1)"; return MPCMP_EINVAL; }
    if (c->quirk_dtau_dT != 0 && c->quirk_dtau_dT != 1) { err = "quirk_dtau_dT is 0 or 1"; return MPCMP_EINVAL; }
    mpcmp_bounds t;
    mpcmp_bounds_from_config(c, &t);
    if (int rc = validate_boxes(&t, err)) return rc;
    if (!(c->lbT <= c->ubT && c->lbT < INFINITY && c->ubT > -INFINITY)) { err = "lbT <= ubT required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    if (int rc = validate_general_rows(&t, c->num_seg, err)) return rc;
    return MPCMP_OK;
}

// per-problem payloads (payload.hpp: the lumping, shared by the host and k_lump_payloads)
int mpcmp::check_payload(const mpcmp_payload *p, std::string &err) {
    if (!(p->mass >= 0.0) || !std::isfinite(p->mass)) { err = "payload mass must be finite and >= 0"; return MPCMP_EINVAL; }
    for (int d = 0; d < 3; d++) if (!std::isfinite(p->com[d])) { err = "payload com must be finite"; return MPCMP_EINVAL; }
    for (int q = 0; q < 9; q++) if (!std::isfinite(p->I[q])) { err = "payload inertia must be finite"; return MPCMP_EINVAL; }
    for (int r = 0; r < 3; r++) {
        if (p->I[4 * r] < 0.0) { err = "payload inertia: negative diagonal entry"; return MPCMP_EINVAL; }
        for (int c = r + 1; c < 3; c++) if (p->I[3 * r + c] != p->I[3 * c + r]) { err = "payload inertia must be symmetric"; return MPCMP_EINVAL; }
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_model_add_payload(const mpcmp_model *m, const mpcmp_payload *p, mpcmp_model *out) {
    if (!m || !p || !out) return MPCMP_EINVAL;
    if (int rc = check_payload(p, g_err)) return rc;
    add_payload(m, p, out);
    return MPCMP_OK;
}

// ---- tool-line moves on the host (include/mpcmp_toolpath.h): one problem through the source the kernels run (toolpath.hpp) ----
extern "C" int mpcmp_tool_line_one(const mpcmp_model *model, int num_seg, const mpcmp_bounds *row, const mpcmp_tool_line_spec *spec, const double *q_start,
                                   const double *R1, const double *p1, double T_in, double *x, double *u, double *T, mpcmp_tool_line *out) {
    using namespace mpcmp_tl;
    if (!model || num_seg < 1 || 3 * num_seg + 1 > TL_MAX_NODES || !row || !q_start || !R1 || !p1 || !x || !u || !T) {
        g_err = "mpcmp_tool_line_one: num_seg in [1, 8] and all pointers (but spec and out) required"; return MPCMP_EINVAL;
    }
    const mpcmp_tool_line_spec sp = spec ? *spec : tl_default_spec();
    if (!tl_spec_ok(sp)) { g_err = "mpcmp_tool_line_one: spec values finite and > 0 (the tool maxima may be +inf), n_sub in [1, 64] required"; return MPCMP_EINVAL; }
    if (const char *why = tl_check_problem(*model, q_start, R1, p1, T_in)) { g_err = std::string("mpcmp_tool_line_one: ") + why; return MPCMP_EINVAL; }
    mpcmp_tool_line rec;
    TlWork work;
    tl_track(*model, num_seg, sp, q_start, R1, p1, T_in, x, 14, 0, 7, u, 7, 0, 0, &rec, work);
    *T = work.T;
    tl_q_excess(x, 14, num_seg, row->lbx, row->ubx, &rec);
    if (out) *out = rec;
    return MPCMP_OK;
}

extern "C" int mpcmp_tool_deviation_one(const mpcmp_model *model, int num_seg, const double *x, const double *R1, const double *p1, int n_pts,
                                        double tol_lin, double tol_ang, mpcmp_tool_dev *out) {
    using namespace mpcmp_tl;
    if (!model || num_seg < 1 || 3 * num_seg + 1 > TL_MAX_NODES || !x || !R1 || !p1 || n_pts < 1 || n_pts > TD_MAX_PTS || !(tol_lin >= 0.0) ||
        !(tol_ang >= 0.0) || !out) {
        g_err = "mpcmp_tool_deviation_one: num_seg in [1, 8], n_pts in [1, 65536], tolerances >= 0 and all pointers required"; return MPCMP_EINVAL;
    }
    TlLine Ln;
    tl_line_of_plan(*model, x, R1, p1, Ln);
    TlDevAcc A;
    tl_dev_init(A);
    for (int i = 0; i <= n_pts; i++) {
        double dl, dp, da;
        tl_dev_sample(*model, Ln, num_seg, x, 14, i, n_pts, &dl, &dp, &da);
        tl_dev_fold(A, i, dl, dp, da, tol_lin, tol_ang);
    }
    *out = tl_dev_record(A, n_pts);
    return MPCMP_OK;
}

// ---- clearance in a moving world on the host (include/mpcmp_moving.h): one plan through the source the kernels run (moving_rule.hpp) ----
extern "C" int mpcmp_track_offset(int n_key, double t0, double dt, const double *P, double tau, double *p) {
    if (!P || !p || n_key < 1 || n_key > MV_MAX_KEYS || !std::isfinite(t0) || !std::isfinite(dt) || !(dt > 0.0) || !std::isfinite(tau)) {
        g_err = "mpcmp_track_offset: n_key in [1, 1024], a finite clock with dt > 0, a finite tau and both pointers required";
        return MPCMP_EINVAL;
    }
    mv_offset(P, mv_place(n_key, t0, dt, tau), p);
    return MPCMP_OK;
}

namespace {
// one plan's tables in the form the kernels stage them
struct MvHost {
    int narm = 0, nseg = 0, nsph = 0, n_obs = 0, n_tracks = 0, n_key = 1, n_grid = 0;
    double t0 = 0.0, dt = 1.0, T = 0.0, T_run = 0.0;
    const mpcmp_sphere *sph = nullptr;
    const mpcmp_obstacle *obs = nullptr;
    const double *off = nullptr, *prof = nullptr;
    std::vector<double> mk, nodes, ok;
    std::vector<int> arm, jnt, tof;
    bool nan = false;
    // world centres cen [nsph][3] at the plan's normalised time s
    void centres(double s, double *cen) const {
        const int nq = 7 * narm;
        double Lg[4], sc[28], fr[2 * 84];
        const int seg = mpcmp_plan::lagrange_segment(nseg, s, Lg);
        for (int j = 0; j < nq; j++) {
            const double q = mpcmp_plan::interp_channel(nodes.data() + j, nq, seg, Lg);
            sc[2 * j] = std::sin(q); sc[2 * j + 1] = std::cos(q);
        }
        for (int a = 0; a < narm; a++) cert_frames(mk.data() + 84 * a, sc + 14 * a, fr + 84 * a);
        for (int i = 0; i < nsph; i++) cert_centre(fr + 84 * arm[i] + 12 * jnt[i], sph[i].c, cen + 3 * i);
    }
    // the clearance of sphere i at the centre c against obstacle o, shifted to the place w of the tracks' clock when it is tracked
    double obstacle(int i, const double *c, int o, const MvPlace &w) const {
        double p[3] = {0.0, 0.0, 0.0};
        if (tof[o] >= 0) mv_offset(off + (size_t)tof[o] * n_key * 3, w, p);
        return clr_sd(obs[o].type, ok.data() + 8 * o, c[0] - p[0], c[1] - p[1], c[2] - p[2]) - sph[i].r;
    }
    double pair(int i, int t, const double *cen) const {
        const double ex = cen[3 * i] - cen[3 * t], ey = cen[3 * i + 1] - cen[3 * t + 1], ez = cen[3 * i + 2] - cen[3 * t + 2];
        return std::sqrt(ex * ex + ey * ey + ez * ez) - sph[i].r - sph[t].r;
    }
};
}  // namespace

// one plan's tables without a timeline: the checks of the sphere tables, then the arrays as the kernels stage them; H->nan: a position node that is
// not finite.  Every statement of the family fills its tables here; what the timed members add is mv_host_setup
static int host_tables(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                       const mpcmp_obstacle *obs, const double *x, MvHost *H) {
    int nsph = 0;
    for (int a = 0; a < narm; a++) { if (n_spheres[a] < 0 || n_spheres[a] > CLR_MAX_SPH) return MPCMP_EINVAL; nsph += n_spheres[a]; }
    if (nsph > 0 && !spheres) return MPCMP_EINVAL;
    for (int s = 0; s < nsph; s++) if (spheres[s].joint < 0 || spheres[s].joint > 6) return MPCMP_EINVAL;
    const int nq = 7 * narm, N = 3 * num_seg + 1;
    H->narm = narm; H->nseg = num_seg; H->nsph = nsph; H->n_obs = n_obs; H->sph = spheres; H->obs = obs;
    H->mk.resize(84 * narm); H->nodes.resize((size_t)nq * N); H->ok.resize(8 * (n_obs > 0 ? n_obs : 1));
    H->arm.resize(nsph); H->jnt.resize(nsph); H->tof.assign(n_obs, -1);
    for (int a = 0; a < narm; a++)
        for (int i = 0; i < 7; i++) {
            for (int c = 0; c < 9; c++) H->mk[84 * a + 12 * i + c] = models[a].R0[i][c];
            for (int c = 0; c < 3; c++) H->mk[84 * a + 12 * i + 9 + c] = models[a].p[i][c];
        }
    for (int k = 0; k < N; k++)
        for (int j = 0; j < nq; j++) { H->nodes[(size_t)k * nq + j] = x[(size_t)k * 2 * nq + j]; if (!std::isfinite(x[(size_t)k * 2 * nq + j])) H->nan = true; }
    for (int a = 0, s = 0; a < narm; a++)
        for (int k = 0; k < n_spheres[a]; k++, s++) { H->arm[s] = a; H->jnt[s] = spheres[s].joint; }
    for (int o = 0; o < n_obs; o++) clr_obs_prepare(obs[o], H->ok.data() + 8 * o);
    return MPCMP_OK;
}

// the checks and tables the timed statements share (the tables of host_tables, the tracks, sol_T and the profile); `who` for the message
static int mv_host_setup(const char *who, const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                         const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt, const double *offsets,
                         const double *x, double T, int n_grid, const double *prof, int n_pts, double margin, int self_gap, const void *out, MvHost *H) {
    if (!models || narm < 1 || narm > 2 || num_seg < 1 || !n_spheres || !x || !out || n_obs < 0 || n_obs > CLR_MAX_OBS || (n_obs > 0 && !obs) ||
        self_gap < 0 || !std::isfinite(margin) || n_pts < 1 || n_pts > 4096 || (prof && (n_grid < 1 || n_grid > MV_MAX_GRID)) || n_tracks < 0 ||
        n_tracks > MV_MAX_TRACKS) {
        g_err = std::string(who) + ": one or two arms, num_seg >= 1, 1 <= n_pts <= 4096, a finite margin, self_gap >= 0, n_obs in [0, 256], n_tracks in "
                "[0, 64], with a profile 1 <= n_grid <= 4096 and all pointers (but prof) required";
        return MPCMP_EINVAL;
    }
    if (n_tracks > 0) {
        bool ok = n_key >= 1 && n_key <= MV_MAX_KEYS && std::isfinite(t0) && std::isfinite(dt) && dt > 0.0 && offsets && (n_obs == 0 || track_of);
        for (int o = 0; ok && o < n_obs; o++) ok = track_of[o] >= -1 && track_of[o] < n_tracks;
        for (size_t e = 0; ok && e < (size_t)n_tracks * n_key * 3; e++) ok = std::isfinite(offsets[e]);
        if (!ok) {
            g_err = std::string(who) + ": n_key in [1, 1024], a finite clock with dt > 0, track_of in [-1, n_tracks) and finite offsets required";
            return MPCMP_EINVAL;
        }
    }
    if (int rc = host_tables(models, narm, num_seg, n_spheres, spheres, n_obs, obs, x, H)) return rc;
    H->n_tracks = n_tracks; H->n_key = n_tracks > 0 ? n_key : 1; H->t0 = t0; H->dt = dt; H->T = T; H->n_grid = n_grid; H->prof = prof; H->off = offsets;
    if (!std::isfinite(T)) H->nan = true;
    if (prof) for (int e = 0; e < 2 * (n_grid + 1); e++) if (!std::isfinite(prof[e])) H->nan = true;
    if (n_tracks > 0) for (int o = 0; o < n_obs; o++) H->tof[o] = mv_track(track_of[o], n_tracks);
    H->T_run = H->nan ? 0.0 : mv_run_time(prof, n_grid, T);
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_timed_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                                         const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt,
                                         const double *offsets, const double *x, double T, int n_grid, const double *prof, double t_start, int n_pts,
                                         double margin, int self_gap, mpcmp_clearance *out) {
    MvHost H;
    if (int rc = mv_host_setup("mpcmp_clearance_timed_one", models, narm, num_seg, n_spheres, spheres, n_obs, obs, track_of, n_tracks, n_key, t0, dt,
                               offsets, x, T, n_grid, prof, n_pts, margin, self_gap, out, &H)) return rc;
    if (H.nan || !std::isfinite(t_start)) { *out = clr_nan_record(); return MPCMP_OK; }
    std::vector<double> cen(3 * (H.nsph > 0 ? H.nsph : 1));
    double best_d = INFINITY;
    unsigned best_k = CLR_NO_PAIR;
    int n_hit = 0, first = -1;
    for (int i = 0; i <= n_pts; i++) {
        double t, s;
        mv_sample(prof, n_grid, T, H.T_run, i, n_pts, &t, &s);
        H.centres(s, cen.data());
        const MvPlace w = mv_place(H.n_key, t0, dt, t_start + t);
        bool hit = false;
        for (int sp = 0; sp < H.nsph; sp++) {
            for (int o = 0; o < n_obs; o++) {
                const double d = H.obstacle(sp, cen.data() + 3 * sp, o, w);
                const unsigned key = clr_pack(i, sp, 0, o);
                if (clr_better(d, key, best_d, best_k)) { best_d = d; best_k = key; }
                hit = hit || d < margin;
            }
            for (int tp = sp + 1; tp < H.nsph; tp++) {
                if (!clr_pair(H.arm[sp], H.jnt[sp], H.arm[tp], H.jnt[tp], self_gap)) continue;
                const double d = H.pair(sp, tp, cen.data());
                const unsigned key = clr_pack(i, sp, 1, tp);
                if (clr_better(d, key, best_d, best_k)) { best_d = d; best_k = key; }
                hit = hit || d < margin;
            }
        }
        if (hit) { if (first < 0) first = i; n_hit++; }
    }
    *out = clr_record(best_d, best_k, first, n_hit, n_pts, H.T_run);
    return MPCMP_OK;
}

extern "C" int mpcmp_start_delay_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                                     const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt, const double *offsets,
                                     const double *x, double T, int n_grid, const double *prof, int K, const double *delays, int check_wait, int n_pts,
                                     double margin, int self_gap, double *d_min_all, mpcmp_start_delay *out) {
    bool ok = K >= 1 && K <= MV_MAX_DELAYS && delays;
    for (int k = 0; ok && k < K; k++) ok = std::isfinite(delays[k]) && delays[k] >= 0.0 && (k == 0 || delays[k] >= delays[k - 1]);
    if (!ok) { g_err = "mpcmp_start_delay_one: 1 <= K <= 256 delays, finite, >= 0 and ascending, required"; return MPCMP_EINVAL; }
    MvHost H;
    if (int rc = mv_host_setup("mpcmp_start_delay_one", models, narm, num_seg, n_spheres, spheres, n_obs, obs, track_of, n_tracks, n_key, t0, dt,
                               offsets, x, T, n_grid, prof, n_pts, margin, self_gap, out, &H)) return rc;
    if (H.nan) { *out = mv_delay_nan(K, d_min_all); return MPCMP_OK; }
    std::vector<double> cen(3 * (H.nsph > 0 ? H.nsph : 1)), dk(K, INFINITY), w0(K, INFINITY);
    double best = INFINITY;          // over the obstacles that stand still and the robot pairs: it does not depend on the delay
    for (int i = 0; i <= n_pts; i++) {
        double t, s;
        mv_sample(prof, n_grid, T, H.T_run, i, n_pts, &t, &s);
        H.centres(s, cen.data());
        const MvPlace none = mv_place(1, 0.0, 1.0, 0.0);
        for (int sp = 0; sp < H.nsph; sp++) {
            for (int o = 0; o < n_obs; o++) if (H.tof[o] < 0) best = std::fmin(best, H.obstacle(sp, cen.data() + 3 * sp, o, none));
            for (int tp = sp + 1; tp < H.nsph; tp++)
                if (clr_pair(H.arm[sp], H.jnt[sp], H.arm[tp], H.jnt[tp], self_gap)) best = std::fmin(best, H.pair(sp, tp, cen.data()));
        }
        for (int k = 0; k < K; k++) {
            const MvPlace w = mv_place(H.n_key, t0, dt, delays[k] + t);
            double dm = INFINITY;
            for (int sp = 0; sp < H.nsph; sp++)
                for (int o = 0; o < n_obs; o++) if (H.tof[o] >= 0) dm = std::fmin(dm, H.obstacle(sp, cen.data() + 3 * sp, o, w));
            dk[k] = std::fmin(dk[k], dm);
            if (i == 0) w0[k] = dm;
        }
    }
    for (int k = 0; k < K; k++) dk[k] = std::fmin(dk[k], best);
    *out = mv_delay_record(K, delays, dk.data(), w0.data(), check_wait, margin, d_min_all);
    return MPCMP_OK;
}

// ---- certified clearance on the host, without a timeline (include/mpcmp_clearance_cert.h) and with one (include/mpcmp_moving_cert.h): one plan
// through the source the kernel runs (clearance_cert.hpp, and moving_cert_rule.hpp on top of it and of moving_rule.hpp) ----
// The search both statements run on the tables of H.  `timed`: the record times are those of the timeline; otherwise tl holds the motion alone
// (no rests, and H no tracks) and a time is cert_time x T, the static member's own product
static void cert_host(const MvHost &H, bool timed, const MvcTimeline &tl, int n_start, double margin, int self_gap, int max_depth, mpcmp_clearance *out,
                      mpcmp_clearance_cert *cert) {
    if (H.nan) {
        *out = clr_nan_record();
        if (cert) *cert = cert_nan_record();
        return;
    }
    const int narm = H.narm, num_seg = H.nseg, nq = 7 * narm, N = 3 * num_seg + 1, nsph = H.nsph, n_obs = H.n_obs;
    const mpcmp_sphere *spheres = H.sph;
    const mpcmp_obstacle *obs = H.obs;
    std::vector<double> reach(7 * (nsph > 0 ? nsph : 1)), cen(3 * (nsph > 0 ? nsph : 1)), Ds(nsph > 0 ? nsph : 1), pm(3 * (H.n_tracks > 0 ? H.n_tracks : 1)),
        Ek(H.n_tracks > 0 ? H.n_tracks : 1);
    for (int s = 0; s < nsph; s++) cert_reach(H.mk.data() + 84 * H.arm[s] + 9, 12, H.jnt[s], spheres[s].c, reach.data() + 7 * s);
    CertBest B;
    std::vector<int> cur(tl.n0), nxt;
    for (int i = 0; i < tl.n0; i++) cur[i] = i;
    for (int l = 0; !cur.empty(); l++) {
        B.depth = l;
        nxt.clear();
        int n_split = 0;
        for (int i : cur) {
            const MvcInterval v = mvc_interval(tl, n_start, l, i);
            const unsigned tk = cert_tkey(l, i);
            for (int k = 0; k < H.n_tracks; k++)
                Ek[k] = mvc_track_bound(H.off + (size_t)k * H.n_key * 3, H.n_key, H.t0, H.dt, tl.tau0 + v.ta, tl.tau0 + v.tm, tl.tau0 + v.tb, pm.data() + 3 * k);
            double dev[14], sc[28], fr[2 * 84];
            for (int j = 0; j < nq; j++) {
                double qm;
                if (v.phase == MVC_MOTION) dev[j] = cert_deviation(H.nodes.data() + j, nq, num_seg, v.v, &qm);
                else { dev[j] = 0.0; qm = H.nodes[(size_t)(v.phase == MVC_HOLD ? (N - 1) * nq : 0) + j]; }
                sc[2 * j] = std::sin(qm); sc[2 * j + 1] = std::cos(qm);
            }
            for (int a = 0; a < narm; a++) cert_frames(H.mk.data() + 84 * a, sc + 14 * a, fr + 84 * a);
            for (int s = 0; s < nsph; s++) {
                Ds[s] = cert_motion(reach.data() + 7 * s, dev + 7 * H.arm[s]);
                cert_centre(fr + 84 * H.arm[s] + 12 * H.jnt[s], spheres[s].c, cen.data() + 3 * s);
            }
            double d_mid = INFINITY, L = INFINITY;
            for (int s = 0; s < nsph; s++) {
                const double *C = cen.data() + 3 * s;
                for (int o = 0; o < n_obs; o++) {
                    const int k = H.tof[o];
                    double d, bound;
                    if (k >= 0) {
                        const double *M = pm.data() + 3 * k;
                        d = clr_sd(obs[o].type, H.ok.data() + 8 * o, C[0] - M[0], C[1] - M[1], C[2] - M[2]) - spheres[s].r;
                        bound = d - Ds[s] - Ek[k];
                    } else {
                        d = clr_sd(obs[o].type, H.ok.data() + 8 * o, C[0], C[1], C[2]) - spheres[s].r;
                        bound = d - Ds[s];
                    }
                    const unsigned long long key = cert_key(tk, s, 0, o);
                    if (cert_better(d, key, B.d, B.k)) { B.d = d; B.k = key; }
                    d_mid = std::fmin(d_mid, d); L = std::fmin(L, bound);
                }
                for (int t = s + 1; t < nsph; t++) {
                    if (!clr_pair(H.arm[s], H.jnt[s], H.arm[t], H.jnt[t], self_gap)) continue;
                    const double d = H.pair(s, t, cen.data());
                    const unsigned long long key = cert_key(tk, s, 1, t);
                    if (cert_better(d, key, B.d, B.k)) { B.d = d; B.k = key; }
                    d_mid = std::fmin(d_mid, d); L = std::fmin(L, d - Ds[s] - Ds[t]);
                }
            }
            B.n_eval++;
            int what = cert_decide(d_mid, L, margin, l, max_depth);
            if (what == CERT_SPLIT_IT) {
                if (n_split < CERT_SPLIT) { n_split++; nxt.push_back(2 * i); nxt.push_back(2 * i + 1); continue; }
                what = CERT_UNDECIDED;          // (the capacity rule)
            }
            if (what == CERT_HIT) { B.n_hit++; if (tk < B.first) B.first = tk; }
            else if (what == CERT_CLEAR) B.n_clear++;
            else B.n_und++;
            const unsigned long long lk = cert_key(tk, 0, 0, 0);
            if (cert_better(L, lk, B.L, B.Lk)) { B.L = L; B.Lk = lk; }
        }
        cur.swap(nxt);
    }
    mpcmp_clearance_cert c;
    cert_records(B, [&](unsigned tkey) { return timed ? mvc_time(tl, tkey) : cert_time(tl.n0, tkey) * tl.T; }, out, &c);
    if (cert) *cert = c;
}

extern "C" int mpcmp_clearance_certified_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                                             const mpcmp_obstacle *obs, const double *x, double T, double margin, int self_gap, int n_start, int max_depth,
                                             mpcmp_clearance *out, mpcmp_clearance_cert *cert) {
    if (!models || narm < 1 || narm > 2 || num_seg < 1 || !n_spheres || !x || !out || n_obs < 0 || n_obs > CLR_MAX_OBS || (n_obs > 0 && !obs) ||
        self_gap < 0 || !std::isfinite(margin) || n_start < 1 || n_start > CERT_CAP || (long)num_seg * n_start > CERT_CAP || max_depth < 0 ||
        max_depth > CERT_MAX_DEPTH) {
        g_err = "mpcmp_clearance_certified_one: one or two arms, num_seg >= 1, n_start >= 1 with num_seg n_start <= 4096, max_depth in [0, 16], a finite "
                "margin, self_gap >= 0, n_obs in [0, 256] and all pointers (but cert) required";
        return MPCMP_EINVAL;
    }
    MvHost H;          // (no tracks, and sol_T is not tested)
    if (int rc = host_tables(models, narm, num_seg, n_spheres, spheres, n_obs, obs, x, &H)) return rc;
    cert_host(H, false, mvc_timeline(num_seg, n_start, 0, T, 0.0, 0.0, 0.0), n_start, margin, self_gap, max_depth, out, cert);
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_certified_timed_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres,
                                                   int n_obs, const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt,
                                                   const double *offsets, const double *x, double T, double t_start, double wait_before,
                                                   double hold_after, double margin, int self_gap, int n_start, int n_rest, int max_depth,
                                                   mpcmp_clearance *out, mpcmp_clearance_cert *cert) {
    if (n_start < 1 || n_start > CERT_CAP || n_rest < 1 || n_rest > CERT_CAP || num_seg < 1 || (long)num_seg * n_start + 2l * n_rest > CERT_CAP ||
        max_depth < 0 || max_depth > CERT_MAX_DEPTH || wait_before < 0.0 || hold_after < 0.0) {
        g_err = "mpcmp_clearance_certified_timed_one: n_start >= 1 and n_rest >= 1 with num_seg n_start + 2 n_rest <= 4096, max_depth in [0, 16], "
                "wait_before >= 0 and hold_after >= 0 required";
        return MPCMP_EINVAL;
    }
    MvHost H;
    if (int rc = mv_host_setup("mpcmp_clearance_certified_timed_one", models, narm, num_seg, n_spheres, spheres, n_obs, obs, track_of, n_tracks, n_key, t0,
                               dt, offsets, x, T, 0, nullptr, 1, margin, self_gap, out, &H)) return rc;
    if (!mvc_times_ok(T, t_start, wait_before, hold_after)) H.nan = true;
    cert_host(H, true, mvc_timeline(num_seg, n_start, n_rest, T, t_start, wait_before, hold_after), n_start, margin, self_gap, max_depth, out, cert);
    return MPCMP_OK;
}

// ---- voxel worlds on the host (include/mpcmp_field.h): the transform, the distance and one configuration through the source the kernels run
// (field_rule.hpp) ----
extern "C" int mpcmp_field_edt(const mpcmp_field_desc *desc, const unsigned char *occ, unsigned *d2) {
    if (!desc || !occ || !d2 || !fld_desc_ok(*desc)) {
        g_err = "mpcmp_field_edt: 1 <= n[d] <= 1024 with at most 2^24 voxels, a finite origin, a finite h > 0 and all pointers required";
        return MPCMP_EINVAL;
    }
    const int n[3] = {desc->n[0], desc->n[1], desc->n[2]};
    const size_t stride[3] = {1, (size_t)n[0], (size_t)n[0] * n[1]}, nv = (size_t)fld_voxels(*desc);
    for (size_t v = 0; v < nv; v++) d2[v] = occ[v] ? 0u : FLD_INF;
    std::vector<unsigned> line(FLD_MAX_DIM);
    // pass x, y, z: every line along the axis through the sweep of fld_minplus, in place by way of a copy of the line
    for (int ax = 0; ax < 3; ax++) {
        const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
        for (int p = 0; p < n[a1]; p++)
            for (int q = 0; q < n[a2]; q++) {
                unsigned *L = d2 + p * stride[a1] + q * stride[a2];
                for (int k = 0; k < n[ax]; k++) line[k] = L[k * stride[ax]];
                for (int j = 0; j < n[ax]; j++) L[j * stride[ax]] = fld_minplus(line.data(), n[ax], j);
            }
    }
    for (size_t v = 0; v < nv; v++) if (d2[v] >= FLD_INF) d2[v] = MPCMP_FIELD_EMPTY;
    return MPCMP_OK;
}

extern "C" int mpcmp_field_sd(const mpcmp_field_desc *desc, const unsigned *d2, const double *x, double *sd, int *voxel) {
    if (!desc || !d2 || !x || !sd || !fld_desc_ok(*desc) || !std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2])) {
        g_err = "mpcmp_field_sd: a valid grid, a finite point and the pointers desc, d2, x and sd required";
        return MPCMP_EINVAL;
    }
    int v;
    *sd = fld_sd(*desc, d2, x[0], x[1], x[2], &v);
    if (voxel) *voxel = v;
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_field_config(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres,
                                            const mpcmp_field_desc *desc, const unsigned *d2, const double *q, double *d_min, int *sphere, int *voxel) {
    if (!models || narm < 1 || narm > 2 || !n_spheres || !q || !d_min || !desc || !d2 || !fld_desc_ok(*desc)) {
        g_err = "mpcmp_clearance_field_config: one or two arms, a valid grid and the pointers models, n_spheres, desc, d2, q and d_min required";
        return MPCMP_EINVAL;
    }
    int nsph = 0;
    for (int a = 0; a < narm; a++) { if (n_spheres[a] < 0 || n_spheres[a] > CLR_MAX_SPH) return MPCMP_EINVAL; nsph += n_spheres[a]; }
    if (nsph > 0 && !spheres) return MPCMP_EINVAL;
    for (int s = 0; s < nsph; s++) if (spheres[s].joint < 0 || spheres[s].joint > 6) return MPCMP_EINVAL;
    for (int j = 0; j < 7 * narm; j++) if (!std::isfinite(q[j])) return MPCMP_EINVAL;
    double best = INFINITY;
    int bs = -1, bv = 0;
    for (int a = 0, s = 0; a < narm; a++) {
        double mk[84], sc[14], fr[84];
        for (int i = 0; i < 7; i++) {
            for (int c = 0; c < 9; c++) mk[12 * i + c] = models[a].R0[i][c];
            for (int c = 0; c < 3; c++) mk[12 * i + 9 + c] = models[a].p[i][c];
            sc[2 * i] = std::sin(q[7 * a + i]); sc[2 * i + 1] = std::cos(q[7 * a + i]);
        }
        cert_frames(mk, sc, fr);
        for (int k = 0; k < n_spheres[a]; k++, s++) {
            double c[3];
            int v;
            cert_centre(fr + 12 * spheres[s].joint, spheres[s].c, c);
            const double d = fld_sd(*desc, d2, c[0], c[1], c[2], &v) - spheres[s].r;
            if (d < best) { best = d; bs = s; bv = v; }      // (ascending spheres: ties stay with the lowest)
        }
    }
    *d_min = best;
    if (sphere) *sphere = bs;
    if (voxel) *voxel = bv;
    return MPCMP_OK;
}

// ---- camera frames on the host (include/mpcmp_frame.h): the filter table, the marker over its three sources and the carver through the source the
// kernels run (frame_rule.hpp) ----
// tab [ns][4] = c_s, R_s^2 of the posture q; false: an argument the rule refuses
static bool frame_table_host(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const double *q, double pad,
                             std::vector<double> *tab) {
    if (!models || narm < 1 || narm > 2 || !n_spheres || !q || !frm_pad_ok(pad)) return false;
    int nsph = 0;
    for (int a = 0; a < narm; a++) { if (n_spheres[a] < 0 || n_spheres[a] > CLR_MAX_SPH) return false; nsph += n_spheres[a]; }
    if (nsph > 0 && !spheres) return false;
    for (int s = 0; s < nsph; s++) if (spheres[s].joint < 0 || spheres[s].joint > 6) return false;
    for (int j = 0; j < 7 * narm; j++) if (!std::isfinite(q[j])) return false;
    tab->assign(4 * (size_t)nsph, 0.0);
    for (int a = 0, s = 0; a < narm; a++) {
        double mk[84], sc[14], fr[84];
        for (int i = 0; i < 7; i++) {
            for (int c = 0; c < 9; c++) mk[12 * i + c] = models[a].R0[i][c];
            for (int c = 0; c < 3; c++) mk[12 * i + 9 + c] = models[a].p[i][c];
            sc[2 * i] = std::sin(q[7 * a + i]); sc[2 * i + 1] = std::cos(q[7 * a + i]);
        }
        cert_frames(mk, sc, fr);
        for (int k = 0; k < n_spheres[a]; k++, s++) frm_entry(fr + 12 * spheres[s].joint, spheres[s].c, spheres[s].r, pad, tab->data() + 4 * s);
    }
    return true;
}
static const char *const FRAME_HOST_ERR = ": one or two arms with their sphere tables and a finite q (or q == NULL), a finite pad >= 0, a valid grid, the "
                                          "data, occ and no flag but MPCMP_FRAME_KEEP required";

extern "C" int mpcmp_frame_spheres(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const double *q, double pad,
                                   double *out) {
    std::vector<double> tab;
    if (!out || !frame_table_host(models, narm, n_spheres, spheres, q, pad, &tab)) {
        g_err = "mpcmp_frame_spheres: one or two arms with their sphere tables, a finite q, a finite pad >= 0 and out required"; return MPCMP_EINVAL;
    }
    for (size_t s = 0; s < tab.size() / 4; s++) {
        for (int c = 0; c < 3; c++) out[4 * s + c] = tab[4 * s + c];
        out[4 * s + 3] = spheres[s].r + pad;
    }
    return MPCMP_OK;
}

// `source`: n items, item i gives its world point (false: INVALID)
template <class Source>
static int frame_mark_host(const char *who, const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres,
                           const mpcmp_field_desc *desc, bool given, int n, Source source, const double *q, double pad, int flags, unsigned char *occ,
                           mpcmp_frame_stats *stats) {
    std::vector<double> tab;
    if (!desc || !fld_desc_ok(*desc) || !given || !occ || !frm_pad_ok(pad) || (flags & ~MPCMP_FRAME_KEEP) ||
        (q && !frame_table_host(models, narm, n_spheres, spheres, q, pad, &tab))) {
        g_err = std::string(who) + FRAME_HOST_ERR; return MPCMP_EINVAL;
    }
    const int ns = (int)(tab.size() / 4);
    if (!(flags & MPCMP_FRAME_KEEP)) std::memset(occ, 0, (size_t)fld_voxels(*desc));
    int count[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        double x[3];
        int code = -1 - FRM_INVALID;
        if (source(i, x)) code = frm_classify(*desc, tab.data(), ns, x);
        if (code >= 0) occ[code] = 1;
        count[frm_class_of(code)]++;
    }
    if (stats) *stats = mpcmp_frame_stats{n, count[FRM_INVALID], count[FRM_OUTSIDE], count[FRM_ROBOT], count[FRM_MARKED], 0, {0, 0}};
    return MPCMP_OK;
}

extern "C" int mpcmp_frame_points_one(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                                      int n_points, const double *points, const double *q, double pad, int flags, unsigned char *occ,
                                      mpcmp_frame_stats *stats) {
    return frame_mark_host("mpcmp_frame_points_one", models, narm, n_spheres, spheres, desc, n_points >= 0 && (n_points == 0 || points), n_points,
                           [&](int i, double *x) { for (int c = 0; c < 3; c++) x[c] = points[3 * (size_t)i + c]; return true; }, q, pad, flags, occ, stats);
}

extern "C" int mpcmp_frame_depth_one(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                                     const mpcmp_camera *cam, const void *depth, int depth_type, const double *q, double pad, int flags,
                                     unsigned char *occ, mpcmp_frame_stats *stats) {
    const bool given = cam && depth && frm_camera_ok(*cam) && (depth_type == MPCMP_DEPTH_U16 || depth_type == MPCMP_DEPTH_F32);
    return frame_mark_host("mpcmp_frame_depth_one", models, narm, n_spheres, spheres, desc, given, given ? cam->width * cam->height : 0,
                           [&](int i, double *x) {
                               if (depth_type == MPCMP_DEPTH_U16) {
                                   const unsigned short d = static_cast<const unsigned short *>(depth)[i];
                                   return frm_pixel(*cam, i % cam->width, i / cam->width, (double)d, frm_raw_ok_u16(d), x);
                               }
                               const float d = static_cast<const float *>(depth)[i];
                               return frm_pixel(*cam, i % cam->width, i / cam->width, (double)d, frm_raw_ok_f32(d), x);
                           }, q, pad, flags, occ, stats);
}

extern "C" int mpcmp_frame_carve_one(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                                     const double *q, double pad, unsigned char *occ, mpcmp_frame_stats *stats) {
    std::vector<double> tab;
    if (!desc || !fld_desc_ok(*desc) || !occ || !frm_pad_ok(pad) || (q && !frame_table_host(models, narm, n_spheres, spheres, q, pad, &tab))) {
        g_err = std::string("mpcmp_frame_carve_one") + FRAME_HOST_ERR; return MPCMP_EINVAL;
    }
    const int ns = (int)(tab.size() / 4), nv = fld_voxels(*desc);
    int cleared = 0;
    for (int v = 0; v < nv; v++)
        if (occ[v] && frm_carved(*desc, tab.data(), ns, v)) { occ[v] = 0; cleared++; }
    if (stats) *stats = mpcmp_frame_stats{0, 0, 0, 0, 0, cleared, {0, 0}};
    return MPCMP_OK;
}

// ---- certified clearance against a voxel world on the host (include/mpcmp_field_cert.h): one plan through the source the kernel runs
// (field_cert_rule.hpp on top of clearance_cert.hpp and field_rule.hpp) ----
extern "C" int mpcmp_clearance_certified_field_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres,
                                                   const mpcmp_field_desc *desc, const unsigned *d2, const double *x, double T, double margin, int n_start,
                                                   int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert) {
    if (!models || narm < 1 || narm > 2 || num_seg < 1 || !n_spheres || !x || !out || !desc || !d2 || !fld_desc_ok(*desc) || !std::isfinite(margin) ||
        n_start < 1 || n_start > CERT_CAP || (long)num_seg * n_start > CERT_CAP || max_depth < 0 || max_depth > CERT_MAX_DEPTH) {
        g_err = "mpcmp_clearance_certified_field_one: one or two arms, num_seg >= 1, n_start >= 1 with num_seg n_start <= 4096, max_depth in [0, 16], a "
                "finite margin, a valid grid and all pointers (but cert) required";
        return MPCMP_EINVAL;
    }
    MvHost H;          // (no obstacles, no tracks, and T is not tested)
    if (int rc = host_tables(models, narm, num_seg, n_spheres, spheres, 0, nullptr, x, &H)) return rc;
    if (H.nan) {
        *out = clr_nan_record();
        if (cert) *cert = cert_nan_record();
        return MPCMP_OK;
    }
    const int nq = 7 * narm, nsph = H.nsph, n0 = num_seg * n_start;
    std::vector<double> reach(7 * (nsph > 0 ? nsph : 1));
    for (int s = 0; s < nsph; s++) cert_reach(H.mk.data() + 84 * H.arm[s] + 9, 12, H.jnt[s], spheres[s].c, reach.data() + 7 * s);
    CertBest B;
    int best_v = 0;
    std::vector<int> cur(n0), nxt;
    for (int i = 0; i < n0; i++) cur[i] = i;
    for (int l = 0; !cur.empty(); l++) {
        B.depth = l;
        nxt.clear();
        int n_split = 0;
        for (int i : cur) {
            const CertInterval v = cert_interval(n0, n_start, l, i);
            const unsigned tk = cert_tkey(l, i);
            double dev[14], sc[28], fr[2 * 84];
            for (int j = 0; j < nq; j++) {
                double qm;
                dev[j] = cert_deviation(H.nodes.data() + j, nq, num_seg, v, &qm);
                sc[2 * j] = std::sin(qm); sc[2 * j + 1] = std::cos(qm);
            }
            for (int a = 0; a < narm; a++) cert_frames(H.mk.data() + 84 * a, sc + 14 * a, fr + 84 * a);
            double d_mid = INFINITY, L = INFINITY;
            for (int s = 0; s < nsph; s++) {
                double c[3];
                int vox;
                cert_centre(fr + 84 * H.arm[s] + 12 * H.jnt[s], spheres[s].c, c);
                const double d = fcert_distance(*desc, d2, c, spheres[s].r, &vox);
                const double D = cert_motion(reach.data() + 7 * s, dev + 7 * H.arm[s]);
                const unsigned long long key = fcert_key(tk, s);
                if (d < INFINITY && cert_better(d, key, B.d, B.k)) { B.d = d; B.k = key; best_v = vox; }
                d_mid = std::fmin(d_mid, d); L = std::fmin(L, d - D);
            }
            B.n_eval++;
            int what = cert_decide(d_mid, L, margin, l, max_depth);
            if (what == CERT_SPLIT_IT) {
                if (n_split < CERT_SPLIT) { n_split++; nxt.push_back(2 * i); nxt.push_back(2 * i + 1); continue; }
                what = CERT_UNDECIDED;          // (the capacity rule)
            }
            if (what == CERT_HIT) { B.n_hit++; if (tk < B.first) B.first = tk; }
            else if (what == CERT_CLEAR) B.n_clear++;
            else B.n_und++;
            const unsigned long long lk = cert_key(tk, 0, 0, 0);
            if (cert_better(L, lk, B.L, B.Lk)) { B.L = L; B.Lk = lk; }
        }
        cur.swap(nxt);
    }
    mpcmp_clearance_cert c;
    cert_records(B, [&](unsigned tkey) { return cert_time(n0, tkey) * T; }, out, &c);
    if (B.k != CERT_NO_PAIR) out->other = best_v;
    if (cert) *cert = c;
    return MPCMP_OK;
}
