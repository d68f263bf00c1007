// mpcmp.hip — C-ABI entry points (include/mpcmp.h) of the MI355X-native batched min-time MPC solver.
// Host logic only orchestrates HIP launches; there is NO CPU fallback: without a HIP device every compute
// entry point fails with MPCMP_ENODEVICE.
#include <hip/hip_runtime.h>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include <algorithm>
#include <array>
#include <functional>
#include <map>

#include "../../include/mpcmp.h"
#include "solver_kernels.hpp"
#include "qp_kernel_v2.hpp"
#include "qp_kernel_v3.hpp"
#ifdef MPCMP_WITH_QP4      /* the measured two-OCPs-per-CU alternative for N = 13 (does not pay): tools/experiments/, built only on request (-DMPCMP_WITH_QP4 -Itools/experiments) */
#include "qp_kernel_v4.hpp"
#endif
#include "qp_kernel_v5.hpp"
#include "multi_kernels.hpp"
#include "kinematics_host.hpp"
#include "jerk_device.hpp"
#include "ik_device.hpp"
#include "payload.hpp"
#include "time_sync.hpp"
#include "clearance.hpp"
#include "limits.hpp"
#include "route.hpp"

#ifdef MPCMP_SPLIT_N25
// the N = 25 kernels live in qp3_n25.hip (built with another scheduler strategy: see there)
namespace mpcmp {
extern template __global__ void k_qp3f<8, 1>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
extern template __global__ void k_qp3f<8, 2>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
extern template __global__ void k_qp3<8, 1>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
extern template __global__ void k_qp3<8, 2>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
}  // namespace mpcmp
#endif

#ifdef MPCMP_SPLIT_N19
// the N = 19 one-arm pair lives in qp5_n19.hip (its own scheduler strategy: see there)
namespace mpcmp {
extern template __global__ void k_qp3f<6, 1, 5>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
extern template __global__ void k_qp5<6>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
}  // namespace mpcmp
#endif

using namespace mpcmp;

struct mpcmp_ctx {
    mpcmp_config cfg;
    int device = 0, max_batch = 0, nseg = 0, narm = 1;
    int N = 0, n = 0, meq = 0, m = 0, mn = 0;      // of the whole OCP (all arms): n = 21 N narm + 1, meq = 14 (N-1) narm, m = meq + 8 N narm
    int nx = 14, nu = 7;                           // state / control entries per node: 14 narm, 7 narm
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t stream_x[3] = {nullptr, nullptr, nullptr};   // further parts of a large solve (see solve_impl)
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // device buffers
    mpcmp_model *d_model = nullptr;   // [narm]
    mpcmp_model model;             // host copy: passed by value to the kernels that run the rigid-body recursions
    // per-problem payloads (mpcmp_set_payloads): d_pmodel [max_batch][narm] = the context's models with row b's payloads lumped in, written by
    // k_lump_payloads from d_pay [max_batch][narm]; both allocated by the first mpcmp_set_payloads.  pay_rows = 0: every problem reads d_model
    mpcmp_model *d_pmodel = nullptr;
    mpcmp_payload *d_pay = nullptr;
    int pay_rows = 0;
    // per-problem final-time windows (mpcmp_set_time_windows): d_tbox [max_batch][2] = (lbT, ubT), allocated by the first call; tw_rows = 0: cfg.lbT / ubT
    double *d_tbox = nullptr;
    int tw_rows = 0;
    // per-problem bounds (mpcmp_set_bounds): d_bnd [max_batch] rows of the six bound tables, allocated by the first setter call; bnd_rows = 0: the
    // tables of cfg for every problem
    mpcmp_bounds *d_bnd = nullptr;
    int bnd_rows = 0;
    // the synchronised solve's buffers (mpcmp_solve_batch_synced*), [max_batch] each, allocated by its first call: group keys, member counts and
    // times, the pass-2 mask (WS::retired of pass 2), the pass-1 status words, rows, T_new and stretched start guess
    int *d_sg_count = nullptr, *d_sg_skip = nullptr, *d_sg_status = nullptr;
    unsigned long long *d_sg_key = nullptr;
    double *d_sg_T = nullptr, *d_sg_rows = nullptr, *d_sg_Tn = nullptr, *d_sg_wx = nullptr, *d_sg_wu = nullptr, *d_sg_wT = nullptr;
    // clearance checks (mpcmp_clearance_batch*): the sphere tables of the arms (host copies; d_clr_sph [128] holds them arm-major, allocated by
    // mpcmp_create), the obstacle sets d_clr_obs [clr_sets][clr_nobs] (allocated and grown by mpcmp_set_obstacles*), the selection's keys
    // ([max_batch], allocated by its first call).  Read by no other entry point
    mpcmp_sphere clr_sph[2][CLR_MAX_SPH];
    int clr_nsph[2] = {0, 0};
    ClrSphere *d_clr_sph = nullptr;
    mpcmp_obstacle *d_clr_obs = nullptr;
    size_t clr_obs_cap = 0;
    int clr_sets = 0, clr_nobs = 0;
    bool clr_ready = false;          // the kernel's dynamic-LDS ceiling is set by the first check, so that a context that never checks never asks for it
    unsigned long long *d_sel_key = nullptr;
    // via-point routes (mpcmp_solve_route_batch*): [max_batch] rows each, allocated by its first call and never afterwards: the leg states and their
    // start guess, and the legs' records when the caller wants none
    double *d_rt_x0 = nullptr, *d_rt_xf = nullptr, *d_rt_wx = nullptr, *d_rt_wu = nullptr, *d_rt_wT = nullptr;
    mpcmp_info *d_rt_info = nullptr;
    int *d_ext_of_int = nullptr, *d_entry_ptr = nullptr;
    uint32_t *d_terms = nullptr;
    WS ws{};
    std::vector<void *> allocs;
    // host-API staging (device side)
    double *d_x0 = nullptr, *d_xf = nullptr, *d_wx = nullptr, *d_wu = nullptr, *d_wT = nullptr;
    double *d_sx = nullptr, *d_su = nullptr, *d_sT = nullptr;
    double *d_ax0 = nullptr, *d_axf = nullptr, *d_awx = nullptr, *d_awu = nullptr, *d_awT = nullptr;   // multi-arm warm start staging
    mpcmp_info *d_info = nullptr;
    uint32_t *d_stream = nullptr;
    Qp2Streams streams{};
    Qp3Pat *d_pat = nullptr;       // sparse K_JC pattern of k_qp3 (num_seg 6, 8), device copy
    double *d_fac = nullptr;       // factor workspace of k_qp3f -> k_qp3: [max_batch][narm][Qp3::FAC]
    Xch xch{nullptr};              // arm-to-arm exchange slots (multi-arm contexts)
    // num_seg 4: second set of structure tables (structure3.hpp order, T bordered out) for the E-free QP kernels (k_qp3f + k_qp4 / k_qp3)
    int *d3_ext_of_int = nullptr, *d3_entry_ptr = nullptr;
    uint32_t *d3_terms = nullptr;
    uint32_t *d_lane4 = nullptr;   // lane-constant table of k_qp4 (qp4_build_lanes)
    int qp13 = 2;                  // QP kernel of num_seg 4: 2 = k_qp2, 3 = k_qp3f + k_qp3, 4 = k_qp3f + k_qp4 (env MPCMP_QP13)
    int qp19 = 5;                  // QP kernel of num_seg 6, one arm: 5 = k_qp3f<6, 1, 5> + k_qp5 (factor resident in registers), 3 = k_qp3f + k_qp3 (env MPCMP_QP19)
    // timing of the dominant kernel (k_qp)
    struct EvPair { hipEvent_t e[2]; };
    std::vector<EvPair> ev;          // at most MAX_EV pairs are ever created; launches beyond that are not timed until the
    size_t ev_used = 0;              // pairs have been folded by mpcmp_kernel_timing
    static constexpr size_t MAX_EV = 4096;
    const char *loop_kernel = "";    // its name: KSel::loop_kernel_name, set with the kernels' LDS limits (prepare_kernels)
    double qp_ms = 0.0;
    int qp_launches = 0;
    bool timing = false;             // off until mpcmp_kernel_timing is first called: a plain solve records no events
    // growable device scratch of the host-pointer entry points (Stage: no hipMalloc per call once it is large enough)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    // receding-horizon state (mpcmp_rh_*)
    int rh_B = 0;
    size_t lam_count = 0;          // doubles in ws.lam (max_batch x (m + n))
    bool rh_first = true;
    hipGraph_t rh_graph = nullptr;
    hipGraphExec_t rh_exec = nullptr;
    double rh_dt = 0.0;
    int *d_retired = nullptr;                    // [max_batch] arrived instances of the receding-horizon loop (k_advance); not re-solved
    unsigned long long *d_rh_count = nullptr;    // [2] re-solves executed, instances retired now (since mpcmp_rh_init)
    hipEvent_t ev_upd[2] = {nullptr, nullptr};   // with_caller_stream: the caller's stream -> ctx->stream, and back
    // diagnostics read from the environment ONCE PER CONTEXT, in mpcmp_create (never process-global state)
    bool force_v1 = false, single_stream = false, debug_occ = false;
    int parts_env = 0;                           // MPCMP_STREAMS: parts of a large batch (0 = automatic, see solve_impl)
};

// the sizes of one problem (all arms): the context's buffers are allocated with them (create_impl) and sliced by them (split)
struct Dims { int N, n, meq, m, mn; };
static constexpr Dims dims_of(int nseg, int narm) {
    const int N = 3 * nseg + 1, n = 21 * N * narm + 1, meq = 14 * (N - 1) * narm, m = meq + 8 * N * narm;
    return {N, n, meq, m, m + n};
}
// ... and that they are the sizes the kernels index with, for every instantiated discretisation
template <int NSEG>
static constexpr bool dims_match() { constexpr Dims d = dims_of(NSEG, 1); using D = Dim<NSEG>; return d.N == D::N && d.n == D::n && d.meq == D::meq && d.m == D::m && d.mn == D::mn; }
template <int NSEG, int NARM>
static constexpr bool dims_match_m() { constexpr Dims d = dims_of(NSEG, NARM); using D = DimM<NSEG, NARM>; return d.N == D::N && d.n == D::n && d.meq == NARM * D::meq && d.m == D::m && d.mn == D::mn; }
static_assert(dims_match<1>() && dims_match<2>() && dims_match<4>() && dims_match<6>(), "Dim<NSEG> and the context's strides differ");
static_assert(dims_match_m<8, 1>() && dims_match_m<6, 2>() && dims_match_m<8, 2>(), "DimM<NSEG, NARM> and the context's strides differ");

// One solve as the launch code sees it: B problems, device pointers, the stream it is enqueued on, and everything that makes it differ from a plain
// mpcmp_solve_batch_device.  A call is built where the solve is asked for and passed down by reference: the context holds no mode of a solve in flight
struct SolveCall {
    int B = 0;
    const double *x0 = nullptr, *xf = nullptr;                      // [B][nx]
    const double *wx = nullptr, *wu = nullptr, *wT = nullptr;       // start guess: all three or none (the built-in initialiser)
    double *sx = nullptr, *su = nullptr, *sT = nullptr;
    mpcmp_info *info = nullptr;
    hipStream_t stream = nullptr;
    int only_qp = 0, reguess = 0;
    bool rh_step = false;              // a step of the receding-horizon driver: its defaults of the start flags, its retired instances, no per-problem time / bound rows
    const double *tw_rows = nullptr;   // final-time rows that override the context's (the second pass of a synchronised solve)
    const int *skip = nullptr;         // problems that are not re-solved (the second pass of a synchronised solve)
    bool capturing = false;            // the stream is being captured into a graph: no timing events
};

// the configuration the kernels of a solve see: the two start flags resolved to 0 / 1.  0 = the library default (off for mpcmp_solve_batch, ON for
// the receding-horizon driver), 1 = on, -1 = off everywhere (include/mpcmp.h)
static mpcmp_config run_config(const mpcmp_ctx *ctx, const SolveCall &c) {
    mpcmp_config cfg = ctx->cfg;
    cfg.qp_warm_start = c.rh_step ? (cfg.qp_warm_start >= 0) : (cfg.qp_warm_start > 0);
    cfg.carry_multipliers = c.rh_step ? (cfg.carry_multipliers >= 0) : (cfg.carry_multipliers > 0);
    return cfg;
}

static thread_local std::string g_err;

// the models the dynamics of a call read: the context's [narm], or the per-problem copies [rows][narm] (problem b, arm a: base + b * stride + a)
static const mpcmp_model *run_models(const mpcmp_ctx *ctx, int *stride) {
    *stride = ctx->pay_rows > 0 ? ctx->narm : 0;
    return ctx->pay_rows > 0 ? ctx->d_pmodel : ctx->d_model;
}
// the final-time rows a solve reads (WS::tbox): the call's own, the context's, or none (cfg.lbT / ubT; always none for the receding-horizon driver)
static const double *run_rows(const mpcmp_ctx *ctx, const SolveCall &c) {
    if (c.tw_rows) return c.tw_rows;
    return (ctx->tw_rows > 0 && !c.rh_step) ? ctx->d_tbox : nullptr;
}
// the bound rows a solve reads (WS::bnd): the context's, or none (the tables of cfg; always none for the receding-horizon driver)
static const mpcmp_bounds *run_bounds(const mpcmp_ctx *ctx, const SolveCall &c) { return (ctx->bnd_rows > 0 && !c.rh_step) ? ctx->d_bnd : nullptr; }
// the problems a solve leaves alone (WS::retired): the arrived instances of the receding-horizon loop, or the call's own mask
static const int *run_retired(const mpcmp_ctx *ctx, const SolveCall &c) { return c.rh_step ? ctx->d_retired : c.skip; }

// the three per-problem row tables of a context: where the count of rows in force lies, and the words of their messages
struct RowTable { int mpcmp_ctx::*rows; const char *what, *setter, *usage; bool refused_in_loop; };
static const RowTable PAYLOAD_ROWS = {&mpcmp_ctx::pay_rows, "payload", "mpcmp_set_payloads", "p given (or 0 with p NULL: clear)", false};
static const RowTable TIME_ROWS = {&mpcmp_ctx::tw_rows, "final-time", "mpcmp_set_time_windows", "lbT and ubT given (or 0 with both NULL: clear)", true};
static const RowTable BOUND_ROWS = {&mpcmp_ctx::bnd_rows, "bound", "mpcmp_set_bounds", "rows given (or 0 with NULL: clear)", true};
// a call for B problems needs a row for each of them (when rows are set)
static int rows_ok(mpcmp_ctx *ctx, int B, const RowTable &t) {
    const int rows = ctx->*t.rows;
    if (rows > 0 && B > rows) {
        ctx->err = "more problems (" + std::to_string(B) + ") than " + t.what + " rows (" + std::to_string(rows) + "): see " + t.setter;
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}
static int solve_rows_ok(mpcmp_ctx *ctx, int B) {
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    if (int rc = rows_ok(ctx, B, TIME_ROWS)) return rc;
    return rows_ok(ctx, B, BOUND_ROWS);
}
static int warm_all_or_none(mpcmp_ctx *ctx, const double *wx, const double *wu, const double *wT) {
    if ((wx != nullptr) != (wu != nullptr) || (wx != nullptr) != (wT != nullptr)) { ctx->err = "warm_x, warm_u, warm_T must be all given or all NULL"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            std::ostringstream os_;                                                           \
            os_ << #call << " failed: " << hipGetErrorString(e_) << " (" << __FILE__ << ":" << __LINE__ << ")"; \
            if (ctx) (ctx)->err = os_.str();                                                  \
            g_err = os_.str();                                                                \
            return MPCMP_ERUNTIME;                                                            \
        }                                                                                     \
    } while (0)

// ------------------------------------------------------------------------------------------------
// configuration helpers (host only)
extern "C" const char *mpcmp_version(void) { return "mpcmp 0.1 (gfx950)"; }

extern "C" int mpcmp_num_nodes(int num_seg) { return 3 * num_seg + 1; }

extern "C" int mpcmp_time_nodes(int num_seg, double *tau) {
    if (num_seg < 1 || !tau) return MPCMP_EINVAL;
    static const double xi[4] = {-1.0, -0.5, 0.5, 1.0};
    for (int s = 0; s < num_seg; s++)
        for (int j = 0; j < 4; j++) tau[3 * s + j] = (s + 0.5 * (xi[j] + 1.0)) / num_seg;
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

// ------------------------------------------------------------------------------------------------
// context
template <typename T>
static int dalloc(mpcmp_ctx *ctx, T **p, size_t count) {
    void *q = nullptr;
    HIPCHK(ctx, hipMalloc(&q, count * sizeof(T)));
    ctx->allocs.push_back(q);
    *p = (T *)q;
    return MPCMP_OK;
}

// the rule of the six bound tables (of the configuration, and of every row of mpcmp_set_bounds): infinite ends are allowed (a row or box switched
// off); NaN, lb > ub and an empty box (lb = +inf or ub = -inf) are not.  A general row narrower than 1e-4 takes rho_eq (oracle/ocp.c: u - l < 1e-4);
// the assembly of k_qp and k_qp2 (num_seg 1, 2, 4) gives every general row the plain rho, so its factor would not be the matrix its iteration uses:
// such rows are supported from num_seg 6 on (k_qp3, k_qp5)
static int validate_boxes(const mpcmp_bounds *t, std::string &err) {
    auto box_ok = [](double lb, double ub) { return lb <= ub && lb < INFINITY && ub > -INFINITY; };
    for (int i = 0; i < 14; i++) if (!box_ok(t->lbx[i], t->ubx[i])) { err = "lbx[" + std::to_string(i) + "] <= ubx[" + std::to_string(i) + "] required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    for (int i = 0; i < 7; i++) if (!box_ok(t->lbu[i], t->ubu[i])) { err = "lbu[" + std::to_string(i) + "] <= ubu[" + std::to_string(i) + "] required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    for (int i = 0; i < 8; i++) if (!box_ok(t->lbg[i], t->ubg[i])) { err = "lbg[" + std::to_string(i) + "] <= ubg[" + std::to_string(i) + "] required (no NaN, no empty box)"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}
static int validate_general_rows(const mpcmp_bounds *t, int num_seg, std::string &err) {
    if (num_seg <= 4)
        for (int i = 0; i < 8; i++)
            if (t->ubg[i] - t->lbg[i] < 1e-4) { err = "num_seg 1, 2 and 4: ubg[" + std::to_string(i) + "] - lbg[" + std::to_string(i) + "] must be >= 1e-4 (narrower general rows need num_seg 6 or 8)"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

static int validate(const mpcmp_config *c, std::string &err) {
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

extern "C" const char *mpcmp_last_error(const mpcmp_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

extern "C" int mpcmp_destroy(mpcmp_ctx *ctx) {
    if (!ctx) return MPCMP_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->rh_exec) (void)hipGraphExecDestroy(ctx->rh_exec);
    if (ctx->rh_graph) (void)hipGraphDestroy(ctx->rh_graph);
    for (void *p : ctx->allocs) (void)hipFree(p);
    for (auto &e : ctx->ev) { (void)hipEventDestroy(e.e[0]); (void)hipEventDestroy(e.e[1]); }
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int k = 0; k < 3; k++) { if (ctx->stream_x[k]) (void)hipStreamDestroy(ctx->stream_x[k]); if (ctx->ev_join[k]) (void)hipEventDestroy(ctx->ev_join[k]); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (auto &e : ctx->ev_upd) if (e) (void)hipEventDestroy(e);
    delete ctx;
    return MPCMP_OK;
}

static int create_impl(const mpcmp_config *cfg, const mpcmp_model *model, int narm, int device, int max_batch, mpcmp_ctx **out);
static int prepare_kernels(mpcmp_ctx *ctx);

extern "C" int mpcmp_create(const mpcmp_config *cfg, const mpcmp_model *model, int device, int max_batch, mpcmp_ctx **out) {
    return create_impl(cfg, model, 1, device, max_batch, out);
}

// Multi-arm robot: `models` points at narm models (independent 7-joint chains on one base; a chain's base placement is folded
// into its first joint placement).  The OCP is the reference's (robot_ocp.hpp:31-213) with NX = 14 narm, NU = 7 narm,
// NG = 8 narm; the arms couple only through the final time.  BASELINE.json configs[3]: narm = 2, num_seg = 8.
extern "C" int mpcmp_create_multi(const mpcmp_config *cfg, const mpcmp_model *models, int narm, int device, int max_batch, mpcmp_ctx **out) {
    if (narm < 1 || narm > 2 || (narm > 1 && !models)) { g_err = "narm must be 1 or 2 (with narm models)"; return MPCMP_EINVAL; }
    return create_impl(cfg, models, narm, device, max_batch, out);
}

static int create_impl(const mpcmp_config *cfg, const mpcmp_model *model, int narm, int device, int max_batch, mpcmp_ctx **out) {
    if (!cfg || !out || max_batch < 1) return MPCMP_EINVAL;
    *out = nullptr;
    if (int rc = validate(cfg, g_err)) return rc;
    if (narm == 2) {
        if (cfg->num_seg != 6 && cfg->num_seg != 8) { g_err = "multi-arm OCPs need num_seg 6 or 8 (k_qp3)"; return MPCMP_EINVAL; }
        if (8 + cfg->qp_iters + 1 + 8 * (cfg->qp_iters / cfg->check_every + 1) > MPCMP_XCH_STRIDE) { g_err = "multi-arm OCPs: qp_iters too large for the exchange slots"; return MPCMP_EINVAL; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device >= ndev) {
        g_err = "no HIP device available: the mpcmp product path has no CPU fallback";
        return MPCMP_ENODEVICE;
    }
    mpcmp_ctx *ctx = new mpcmp_ctx();
    ctx->cfg = *cfg; ctx->device = device; ctx->max_batch = max_batch; ctx->nseg = cfg->num_seg; ctx->narm = narm;
    ctx->nx = 14 * narm; ctx->nu = 7 * narm;
    const Dims d = dims_of(cfg->num_seg, narm);
    ctx->N = d.N; ctx->n = d.n; ctx->meq = d.meq; ctx->m = d.m; ctx->mn = d.mn;
    auto fail = [&](int rc) { g_err = ctx->err; mpcmp_destroy(ctx); return rc; };
#define TRY(x) do { int rc_ = (x); if (rc_) return fail(rc_); } while (0)
#define HIPTRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return fail(MPCMP_ERUNTIME); } } while (0)
    HIPTRY(hipSetDevice(device));
    HIPTRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    for (int k = 0; k < 3; k++) {
        HIPTRY(hipStreamCreateWithFlags(&ctx->stream_x[k], hipStreamNonBlocking));
        HIPTRY(hipEventCreateWithFlags(&ctx->ev_join[k], hipEventDisableTiming));
    }
    HIPTRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    for (auto &e : ctx->ev_upd) HIPTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    mpcmp_model mdl[2];
    for (int a = 0; a < narm; a++) { if (model) mdl[a] = model[a]; else mpcmp_default_model(&mdl[a]); }
    TRY(dalloc(ctx, &ctx->d_model, narm));
    HIPTRY(hipMemcpy(ctx->d_model, mdl, sizeof(mpcmp_model) * narm, hipMemcpyHostToDevice));
    ctx->model = mdl[0];
    StructureTables tab;
    // k_qp3 / k_qp4: per-arm tables with T bordered out (structure3.hpp), in ELL form
    auto build_v3 = [&](int nseg, StructureTables &tb, Qp3Pat &pat) -> bool {
        Tables3 t3;
        if (!build_tables3(nseg, t3)) return false;
        tb.nseg = t3.nseg; tb.ext_of_int = t3.ext_of_int; pat = t3.pat;
        // term lists in ELL form [term index][entry] (entry stride padded to 64): consecutive threads assemble consecutive entries,
        // so every load of a term word is one coalesced 256-byte request per wave (the per-entry lists of the CSR form cost a
        // cache line per 4-byte word, and every workgroup of the launch reads the same table: 0.47 M cycles per factorisation)
        const int E = (int)t3.entry_ptr.size() - 1, EP = (E + 63) / 64 * 64;
        // (kappa, the (T, T) entry, has one term per row of A: the kernel sums it by a workgroup reduction instead)
        const int e_kap = nseg * 1225 + 28 + nseg * 196 + nseg * 98 + 98 + 21 * (3 * nseg + 1);      // Dim3<nseg>::eKap
        int tmax = 0;
        for (int e = 0; e < E; e++) if (e != e_kap) tmax = std::max(tmax, t3.entry_ptr[e + 1] - t3.entry_ptr[e]);
        tb.entry_ptr.assign(EP, 0);
        tb.terms.assign((size_t)tmax * EP, 0xFFFFFFFFu);
        // Slots instead of entries: inside each of the two assembly calls' ranges ([0, EA): everything but K_II; [EA, E): K_II) the
        // entries are sorted by the length of their term lists, longest first, so that the 64 lanes of a wave (consecutive slots)
        // walk lists of (nearly) equal length.  In entry order a wave executed every step of its longest list for all of its 10 - 13
        // entries per lane: 140 term evaluations per lane for 32 terms.  tb.entry_ptr[slot] = count | entry << 8.
        const int EA = e_kap + 1;
        auto count_of = [&](int e) { return e == e_kap ? 0 : t3.entry_ptr[e + 1] - t3.entry_ptr[e]; };
        for (int part = 0; part < 2; part++) {
            const int lo = part ? EA : 0, hi = part ? E : EA;
            std::vector<int> order(hi - lo);
            for (int e = lo; e < hi; e++) order[e - lo] = e;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count_of(a) > count_of(b); });
            for (int k = 0; k < hi - lo; k++) {
                const int slot = lo + k, e = order[k], c = count_of(e);
                tb.entry_ptr[slot] = c | (e << 8);
                for (int t = 0; t < c; t++) tb.terms[(size_t)t * EP + slot] = t3.terms[t3.entry_ptr[e] + t];
            }
        }
        return true;
    };
    auto fac_doubles = [](int nseg) -> size_t { return nseg == 4 ? std::max<size_t>(Qp3<4>::FAC, Qp4Fac<4>::FAC) : (nseg == 6 ? std::max<size_t>(Qp3<6>::FAC, Qp5Fac<6>::FAC) : Qp3<8>::FAC); };
    if (cfg->num_seg == 6 && narm == 1) {
        if (const char *e = std::getenv("MPCMP_QP19")) ctx->qp19 = std::atoi(e);
        if (ctx->qp19 != 3 && ctx->qp19 != 5) { ctx->err = "MPCMP_QP19 must be 3 (k_qp3) or 5 (k_qp5)"; return fail(MPCMP_EINVAL); }
    }
    if (cfg->num_seg >= 6) {
        Qp3Pat pat;
        if (!build_v3(cfg->num_seg, tab, pat)) { ctx->err = "internal: structure table generation failed"; return fail(MPCMP_EINVAL); }
        TRY(dalloc(ctx, &ctx->d_fac, (size_t)max_batch * narm * fac_doubles(cfg->num_seg)));
        TRY(dalloc(ctx, &ctx->d_pat, 1));
        HIPTRY(hipMemcpy(ctx->d_pat, &pat, sizeof(Qp3Pat), hipMemcpyHostToDevice));
    } else if (!build_tables(cfg->num_seg, tab)) { ctx->err = "internal: structure table generation failed"; return fail(MPCMP_EINVAL); }
    TRY(dalloc(ctx, &ctx->d_ext_of_int, tab.ext_of_int.size()));
    TRY(dalloc(ctx, &ctx->d_entry_ptr, tab.entry_ptr.size()));
    TRY(dalloc(ctx, &ctx->d_terms, tab.terms.size()));
    HIPTRY(hipMemcpy(ctx->d_ext_of_int, tab.ext_of_int.data(), tab.ext_of_int.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(ctx->d_entry_ptr, tab.entry_ptr.data(), tab.entry_ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(ctx->d_terms, tab.terms.data(), tab.terms.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    const size_t B = max_batch, N = ctx->N, n = ctx->n, mn = ctx->mn;
    WS &w = ctx->ws;
    w.model = ctx->d_model; w.ext_of_int = ctx->d_ext_of_int; w.entry_ptr = ctx->d_entry_ptr; w.terms = ctx->d_terms;
    TRY(dalloc(ctx, &w.z, B * n)); TRY(dalloc(ctx, &w.lam, B * mn)); TRY(dalloc(ctx, &w.ceq, B * ctx->meq));
    HIPTRY(hipMemset(w.lam, 0, sizeof(double) * B * mn));        // (mpcmp_config.carry_multipliers: a fresh context starts every slot from lambda = 0)
    ctx->lam_count = B * mn;
    TRY(dalloc(ctx, &w.g, B * 8 * N * narm)); TRY(dalloc(ctx, &w.Gk, B * N * 176 * narm)); TRY(dalloc(ctx, &w.p, B * n));
    TRY(dalloc(ctx, &w.y, B * mn)); TRY(dalloc(ctx, &w.qpit, B)); TRY(dalloc(ctx, &w.perm, B)); TRY(dalloc(ctx, &w.okey, B)); TRY(dalloc(ctx, &w.done, 4));
    HIPTRY(hipMemset(w.done, 0, 4 * sizeof(int))); TRY(dalloc(ctx, &w.qp_total, B));
    TRY(dalloc(ctx, &w.status, B)); HIPTRY(hipMemset(w.status, 0, sizeof(*w.status) * B)); TRY(dalloc(ctx, &w.alpha, B)); TRY(dalloc(ctx, &w.dbg, (size_t)B * MPCMP_DBG_WORDS));
    const size_t nx = ctx->nx, nu = ctx->nu;
    TRY(dalloc(ctx, &ctx->d_x0, B * nx)); TRY(dalloc(ctx, &ctx->d_xf, B * nx));
    TRY(dalloc(ctx, &ctx->d_wx, B * nx * N)); TRY(dalloc(ctx, &ctx->d_wu, B * nu * N)); TRY(dalloc(ctx, &ctx->d_wT, B));
    TRY(dalloc(ctx, &ctx->d_sx, B * nx * N)); TRY(dalloc(ctx, &ctx->d_su, B * nu * N)); TRY(dalloc(ctx, &ctx->d_sT, B));
    TRY(dalloc(ctx, &ctx->d_info, B));
    if (narm == 2) {
        TRY(dalloc(ctx, &ctx->xch.buf, B * 2 * MPCMP_XCH_STRIDE));
        // per-arm staging of the warm-start generator: states, node trajectories, durations of B * narm arm problems
        TRY(dalloc(ctx, &ctx->d_ax0, B * nx)); TRY(dalloc(ctx, &ctx->d_axf, B * nx));
        TRY(dalloc(ctx, &ctx->d_awx, B * nx * N)); TRY(dalloc(ctx, &ctx->d_awu, B * nu * N)); TRY(dalloc(ctx, &ctx->d_awT, B * narm));
    }
    if (cfg->num_seg == 2 || cfg->num_seg == 4) {
        AsmStreams as;
        const int GS = cfg->num_seg == 4 ? Qp2<4>::GS : Qp2<2>::GS, RSv = Qp2<4>::RS;
        if (!build_streams(cfg->num_seg, 1024, Qp2<4>::HS, GS, RSv, as)) { ctx->err = "internal: assembly stream generation failed"; return fail(MPCMP_EINVAL); }
        TRY(dalloc(ctx, &ctx->d_stream, as.words.size()));
        HIPTRY(hipMemcpy(ctx->d_stream, as.words.data(), as.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        ctx->streams.words = ctx->d_stream; ctx->streams.npass = as.npass;
        for (int p = 0; p < 8; p++) { ctx->streams.off[p] = as.off[p]; ctx->streams.W[p] = as.W[p]; }
        ctx->streams.split_dst = as.split_dst; ctx->streams.split_scr = as.split_scr; ctx->streams.split_n = as.split_n;
    }
    if (cfg->num_seg == 4) {
        if (const char *e = std::getenv("MPCMP_QP13")) ctx->qp13 = std::atoi(e);
        if (ctx->qp13 != 2 && ctx->qp13 != 3 && ctx->qp13 != 4) { ctx->err = "MPCMP_QP13 must be 2 (k_qp2), 3 (k_qp3) or 4 (k_qp4, experimental: slower than k_qp2)"; return fail(MPCMP_EINVAL); }
#ifndef MPCMP_WITH_QP4
        if (ctx->qp13 == 4) { ctx->err = "MPCMP_QP13=4: this library was built without k_qp4 (experimental kernel: rebuild with -DMPCMP_WITH_QP4 -Itools/experiments)"; return fail(MPCMP_EINVAL); }
#endif
        if (ctx->qp13 != 2 && std::getenv("MPCMP_FORCE_V1")) { ctx->err = "MPCMP_FORCE_V1 and MPCMP_QP13 != 2 exclude each other"; return fail(MPCMP_EINVAL); }
        if (ctx->qp13 != 2) {
            StructureTables t4;
            Qp3Pat pat;
            if (!build_v3(4, t4, pat)) { ctx->err = "internal: structure table generation failed"; return fail(MPCMP_EINVAL); }
            TRY(dalloc(ctx, &ctx->d3_ext_of_int, t4.ext_of_int.size()));
            TRY(dalloc(ctx, &ctx->d3_entry_ptr, t4.entry_ptr.size()));
            TRY(dalloc(ctx, &ctx->d3_terms, t4.terms.size()));
            HIPTRY(hipMemcpy(ctx->d3_ext_of_int, t4.ext_of_int.data(), t4.ext_of_int.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPTRY(hipMemcpy(ctx->d3_entry_ptr, t4.entry_ptr.data(), t4.entry_ptr.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPTRY(hipMemcpy(ctx->d3_terms, t4.terms.data(), t4.terms.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            TRY(dalloc(ctx, &ctx->d_fac, (size_t)max_batch * fac_doubles(4)));
            TRY(dalloc(ctx, &ctx->d_pat, 1));
            HIPTRY(hipMemcpy(ctx->d_pat, &pat, sizeof(Qp3Pat), hipMemcpyHostToDevice));
#ifdef MPCMP_WITH_QP4
            std::vector<uint32_t> lane4((size_t)Qp4<4>::NF * Qp4<4>::NT);
            qp4_build_lanes<4>(pat, t4.ext_of_int.data(), lane4.data());
            TRY(dalloc(ctx, &ctx->d_lane4, lane4.size()));
            HIPTRY(hipMemcpy(ctx->d_lane4, lane4.data(), lane4.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
#endif
        }
    }
    TRY(dalloc(ctx, &ctx->d_retired, B)); HIPTRY(hipMemset(ctx->d_retired, 0, sizeof(int) * B));
    TRY(dalloc(ctx, &ctx->d_rh_count, 2)); HIPTRY(hipMemset(ctx->d_rh_count, 0, 2 * sizeof(unsigned long long)));
    // diagnostics (generic kernel everywhere, stream count, occupancy report): read here, per context
    ctx->force_v1 = std::getenv("MPCMP_FORCE_V1") != nullptr;
    ctx->single_stream = std::getenv("MPCMP_SINGLE_STREAM") != nullptr;
    ctx->debug_occ = std::getenv("MPCMP_DEBUG_OCC") != nullptr;
    if (const char *e = std::getenv("MPCMP_STREAMS")) ctx->parts_env = std::atoi(e);
    TRY(prepare_kernels(ctx));
    TRY(dalloc(ctx, &ctx->d_clr_sph, 2 * CLR_MAX_SPH));
#undef TRY
#undef HIPTRY
    *out = ctx;
    return MPCMP_OK;
}

// a captured receding-horizon step holds what it was captured with as kernel arguments (the configuration by value, the model pointer and stride):
// whoever changes one of them drops the graph, and the next mpcmp_rh_run with use_graph captures again
static void drop_rh_graph(mpcmp_ctx *ctx) {
    if (ctx->rh_exec) { (void)hipGraphExecDestroy(ctx->rh_exec); ctx->rh_exec = nullptr; }
    if (ctx->rh_graph) { (void)hipGraphDestroy(ctx->rh_graph); ctx->rh_graph = nullptr; }
}

extern "C" int mpcmp_set_config(mpcmp_ctx *ctx, const mpcmp_config *cfg) {
    if (!ctx || !cfg) return MPCMP_EINVAL;
    if (cfg->num_seg != ctx->nseg) { ctx->err = "num_seg cannot change after mpcmp_create"; return MPCMP_EINVAL; }
    if (int rc = validate(cfg, ctx->err)) return rc;
    if (ctx->narm == 2 && 8 + cfg->qp_iters + 1 + 8 * (cfg->qp_iters / cfg->check_every + 1) > MPCMP_XCH_STRIDE) {
        ctx->err = "multi-arm OCPs: qp_iters too large for the exchange slots"; return MPCMP_EINVAL;
    }
    ctx->cfg = *cfg;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// what the *_device setters and mpcmp_rh_update_device share: body(ctx->stream) runs after the caller's work on its stream (which writes the inputs) and
// the context's own (solves that read what body replaces), before the context's later work; the caller's later work waits for body's reads of its buffers
template <typename F>
static int with_caller_stream(mpcmp_ctx *ctx, void *hip_stream, F body) {
    hipStream_t cs = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipEventRecord(ctx->ev_upd[0], cs));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upd[0], 0));
    if (int rc = body(ctx->stream)) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev_upd[1], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(cs, ctx->ev_upd[1], 0));
    return MPCMP_OK;
}

// the front half of the checks of the three row setters (host and device variant alike).  given / none: every row pointer of the call is set / is NULL
static int rows_check(mpcmp_ctx *ctx, const RowTable &t, int n, bool given, bool none) {
    if (!ctx) { g_err = std::string(t.setter) + ": no context"; return MPCMP_EINVAL; }
    if (t.refused_in_loop && ctx->rh_B > 0) {
        ctx->err = std::string(t.setter) + ": the receding-horizon driver does not read " + t.what + " rows (a loop is running)"; return MPCMP_EINVAL;
    }
    if (n == 0 && none) return MPCMP_OK;
    if (n < 1 || n > ctx->max_batch || !given) { ctx->err = std::string(t.setter) + ": n must be in [1, max_batch] with " + t.usage; return MPCMP_EINVAL; }
    return MPCMP_OK;
}
// first use of a row table: [max_batch] rows of `per_row` entries
template <typename T>
static int rows_alloc(mpcmp_ctx *ctx, T **p, size_t per_row) {
    if (*p) return MPCMP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return dalloc(ctx, p, per_row * ctx->max_batch);
}

// ------------------------------------------------------------------------------------------------
// per-problem payloads (payload.hpp: the lumping, shared by the host and k_lump_payloads)
static int check_payload(const mpcmp_payload *p, std::string &err) {
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

// n rows of narm payloads at d_p (device) -> ctx->d_pmodel on stream st; the scalar checks are the caller's
static int payloads_enqueue(mpcmp_ctx *ctx, int n, const mpcmp_payload *d_p, hipStream_t st) {
    const int threads = n * ctx->narm;
    hipLaunchKernelGGL(k_lump_payloads, dim3((threads + 255) / 256), dim3(256), 0, st, (const mpcmp_model *)ctx->d_model, ctx->narm, n, d_p, ctx->d_pmodel);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

// (payload rows may change while a receding-horizon loop runs, as long as every instance keeps one; the setters then drop the captured step)
static int payloads_check(mpcmp_ctx *ctx, int n, const mpcmp_payload *p) {
    if (int rc = rows_check(ctx, PAYLOAD_ROWS, n, p != nullptr, !p)) return rc;
    if (n == 0) return MPCMP_OK;
    if (ctx->rh_B > 0 && n < ctx->rh_B) { ctx->err = "mpcmp_set_payloads: fewer rows than the instances of the receding-horizon loop"; return MPCMP_EINVAL; }
    if (int rc = rows_alloc(ctx, &ctx->d_pmodel, ctx->narm)) return rc;      // (1,472 + 104 B per arm)
    return rows_alloc(ctx, &ctx->d_pay, ctx->narm);
}

extern "C" int mpcmp_set_payloads(mpcmp_ctx *ctx, int n, const mpcmp_payload *p) {
    if (int rc = payloads_check(ctx, n, p)) return rc;
    if (n > 0)
        for (int i = 0; i < n * ctx->narm; i++)
            if (int rc = check_payload(p + i, ctx->err)) { ctx->err = "mpcmp_set_payloads: row " + std::to_string(i / ctx->narm) + ": " + ctx->err; return rc; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n > 0) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_pay, p, sizeof(mpcmp_payload) * n * ctx->narm, hipMemcpyHostToDevice, st));
        if (int rc = payloads_enqueue(ctx, n, ctx->d_pay, st)) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->pay_rows = n;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

extern "C" int mpcmp_set_payloads_device(mpcmp_ctx *ctx, int n, const mpcmp_payload *d_p, void *hip_stream) {
    if (int rc = payloads_check(ctx, n, d_p)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n > 0)
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) { return payloads_enqueue(ctx, n, d_p, st); })) return rc;
    ctx->pay_rows = n;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// per-problem final-time windows
static int time_windows_check(mpcmp_ctx *ctx, int n, const double *lb, const double *ub) {
    if (int rc = rows_check(ctx, TIME_ROWS, n, lb && ub, !lb && !ub)) return rc;
    return n > 0 ? rows_alloc(ctx, &ctx->d_tbox, 2) : MPCMP_OK;
}

extern "C" int mpcmp_set_time_windows(mpcmp_ctx *ctx, int n, const double *lbT, const double *ubT) {
    if (int rc = time_windows_check(ctx, n, lbT, ubT)) return rc;
    std::vector<double> rows((size_t)2 * n);
    for (int i = 0; i < n; i++) {
        // the rule validate() applies to the configuration's pair (no NaN, lb <= ub, not empty), and lbT >= 0
        if (!(lbT[i] <= ubT[i] && lbT[i] < INFINITY && ubT[i] > -INFINITY && lbT[i] >= 0.0)) {
            ctx->err = "mpcmp_set_time_windows: row " + std::to_string(i) + ": 0 <= lbT <= ubT required (no NaN, no empty window)";
            return MPCMP_EINVAL;
        }
        rows[2 * i] = lbT[i]; rows[2 * i + 1] = ubT[i];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n > 0) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_tbox, rows.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->tw_rows = n;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_time_windows_device(mpcmp_ctx *ctx, int n, const double *d_lbT, const double *d_ubT, void *hip_stream) {
    if (int rc = time_windows_check(ctx, n, d_lbT, d_ubT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n > 0)
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
                HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_tbox, 2 * sizeof(double), d_lbT, sizeof(double), sizeof(double), n, hipMemcpyDeviceToDevice, st));
                HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_tbox + 1, 2 * sizeof(double), d_ubT, sizeof(double), sizeof(double), n, hipMemcpyDeviceToDevice, st));
                return MPCMP_OK;
            })) return rc;
    ctx->tw_rows = n;
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// per-problem bounds
static int bounds_check(mpcmp_ctx *ctx, int n, const mpcmp_bounds *rows) {
    if (int rc = rows_check(ctx, BOUND_ROWS, n, rows != nullptr, !rows)) return rc;
    return n > 0 ? rows_alloc(ctx, &ctx->d_bnd, 1) : MPCMP_OK;
}

extern "C" int mpcmp_set_bounds(mpcmp_ctx *ctx, int n, const mpcmp_bounds *rows) {
    if (int rc = bounds_check(ctx, n, rows)) return rc;
    for (int i = 0; i < n; i++) {
        std::string why;
        if (validate_boxes(rows + i, why) || validate_general_rows(rows + i, ctx->nseg, why)) { ctx->err = "mpcmp_set_bounds: row " + std::to_string(i) + ": " + why; return MPCMP_EINVAL; }
    }
    if (n > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_bnd, rows, sizeof(mpcmp_bounds) * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->bnd_rows = n;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_bounds_device(mpcmp_ctx *ctx, int n, const mpcmp_bounds *d_rows, void *hip_stream) {
    if (int rc = bounds_check(ctx, n, d_rows)) return rc;
    if (n > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
                HIPCHK(ctx, hipMemcpyAsync(ctx->d_bnd, d_rows, sizeof(mpcmp_bounds) * n, hipMemcpyDeviceToDevice, st));
                return MPCMP_OK;
            })) return rc;
    }
    ctx->bnd_rows = n;
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// launches
template <typename K>
static int set_lds(mpcmp_ctx *ctx, K kern, size_t bytes) {
    HIPCHK(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MPCMP_OK;
}

static hipEvent_t *next_events(mpcmp_ctx *ctx) {
    if (ctx->ev_used == ctx->ev.size()) {
        if (ctx->ev.size() >= mpcmp_ctx::MAX_EV) return nullptr;      // bounded: untimed until the caller folds the pairs
        mpcmp_ctx::EvPair p;
        if (hipEventCreate(&p.e[0]) != hipSuccess) return nullptr;
        if (hipEventCreate(&p.e[1]) != hipSuccess) { (void)hipEventDestroy(p.e[0]); return nullptr; }
        ctx->ev.push_back(p);
    }
    return ctx->ev[ctx->ev_used++].e;
}

// Kernel selection of a single-arm context (compile-time candidates, run-time choice by discretisation and the context's diagnostics)
template <int NSEG>
struct KSel {
    static constexpr bool V2C = (NSEG == 2 || NSEG == 4);      // role-specialised 1024-thread QP kernel
    static constexpr bool V3T = (NSEG >= 4);                   // k_qp3 instantiated (num_seg 4: diagnostics, MPCMP_QP13=3)
    static constexpr int N3 = V3T ? NSEG : 6, N2 = V2C ? NSEG : 4, N1 = (NSEG >= 6) ? 1 : NSEG;
    bool V3C, V4, V2, V5;
    explicit KSel(const mpcmp_ctx *ctx) {
        V3C = NSEG >= 6 || (NSEG == 4 && ctx->qp13 == 3);      // k_qp3: T bordered out, E-free interior solve (N = 19, 25)
        V4 = NSEG == 4 && ctx->qp13 == 4;                       // k_qp3f<4, 1, 4> + k_qp4: two OCPs per CU
        V2 = V2C && !ctx->force_v1 && !V3C && !V4;
        V5 = NSEG == 6 && ctx->qp19 == 5;
    }
    // the kernel that runs the ADMM loop, by the order of preference of solve_impl's launches
    const char *loop_kernel_name() const { return V4 ? "k_qp4" : V5 ? "k_qp5" : V3C ? "k_qp3" : V2 ? "k_qp2" : "k_qp"; }
};

// dynamic-LDS limits of every kernel a context of this discretisation can launch: set ONCE, in mpcmp_create
template <int NSEG>
static int prepare_impl(mpcmp_ctx *ctx) {
    using S = KSel<NSEG>;
    const S k(ctx);
    ctx->loop_kernel = k.loop_kernel_name();
    if (int rc = set_lds(ctx, k_init<NSEG>, InitLds<NSEG>::size * sizeof(double))) return rc;
    if (int rc = set_lds(ctx, k_step<NSEG>, StepLds<NSEG>::size * sizeof(double))) return rc;
    if (k.V3C) {
        if (int rc = set_lds(ctx, k_qp3<S::N3, 1>, Qp3<S::N3>::sizeL * sizeof(double))) return rc;
        if (int rc = set_lds(ctx, k_qp3f<S::N3, 1>, Qp3<S::N3>::sizeF * sizeof(double))) return rc;
    }
    if (k.V5) {
        if (int rc = set_lds(ctx, k_qp5<6>, Qp5<6>::size5 * sizeof(double))) return rc;
        if (int rc = set_lds(ctx, k_qp3f<6, 1, 5>, Qp3<6>::sizeF * sizeof(double))) return rc;
    }
#ifdef MPCMP_WITH_QP4
    if (k.V4) {
        const size_t l_qp4 = Qp4<4>::size * sizeof(double);
        if (int rc = set_lds(ctx, k_qp4<4>, l_qp4)) return rc;
        if (int rc = set_lds(ctx, k_qp3f<4, 1, 4>, Qp3<4>::sizeF * sizeof(double))) return rc;
        if (ctx->debug_occ) {
            int nb = -1;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_qp4<4>, 384, l_qp4);
            std::fprintf(stderr, "k_qp4: %zu B of dynamic LDS, %d workgroups per CU\n", l_qp4, nb);
        }
    }
#endif
    if (k.V2) { if (int rc = set_lds(ctx, k_qp2<S::N2>, Qp2<S::N2>::size * sizeof(double))) return rc; }
    else if (!k.V3C && !k.V4) { if (int rc = set_lds(ctx, k_qp<S::N1>, QpLds<S::N1>::size * sizeof(double))) return rc; }
    return MPCMP_OK;
}

// ---- the parts of a solve ----
// A large batch is solved as parts on as many streams (why: solve_impl).  A part is a contiguous range of the call's problems with every per-problem
// pointer of the workspace, the exchange slots, the start guess and the outputs moved to its first problem
struct Part {
    int b0, B;
    hipStream_t stream;
    WS ws;
    Xch xch;
    const double *wx, *wu, *wT;
    double *sx, *su, *sT;
    mpcmp_info *info;
};
struct Parts {
    int n = 0;
    Part p[4];
    const Part *begin() const { return p; }
    const Part *end() const { return p + n; }
};

static Parts split(const mpcmp_ctx *ctx, const SolveCall &c, int nparts) {
    WS w = ctx->ws;
    w.x0 = c.x0; w.xf = c.xf;
    w.model = run_models(ctx, &w.mstride);
    w.retired = run_retired(ctx, c);
    w.tbox = run_rows(ctx, c);
    w.bnd = run_bounds(ctx, c);
    if (c.rh_step) { w.alt_x = ctx->d_wx; w.alt_u = ctx->d_wu; w.alt_T = ctx->d_wT; }
    const size_t nx = ctx->nx, nu = ctx->nu, N = ctx->N, n = ctx->n, mn = ctx->mn, meq = ctx->meq, narm = ctx->narm;
    const hipStream_t streams[4] = {c.stream, ctx->stream_x[0], ctx->stream_x[1], ctx->stream_x[2]};
    Parts ps;
    ps.n = nparts;
    for (int h = 0, acc = 0; h < nparts; h++) {
        Part &q = ps.p[h];
        q.b0 = acc; q.B = (c.B - acc + (nparts - h) - 1) / (nparts - h); q.stream = streams[h];
        acc += q.B;
        const size_t b0 = (size_t)q.b0;
        WS v = w;
        v.x0 += nx * b0; v.xf += nx * b0; v.z += n * b0; v.lam += mn * b0; v.ceq += meq * b0; v.g += 8 * N * narm * b0;
        v.Gk += 176 * N * narm * b0; v.p += n * b0; v.y += mn * b0; v.qpit += b0; v.perm += b0; v.okey += b0; v.done += h;
        v.qp_total += b0; v.status += b0; v.alpha += b0; v.dbg += (size_t)MPCMP_DBG_WORDS * b0;
        v.model += (size_t)v.mstride * b0;      // (the payload row is the problem's index in the whole batch, not in its part)
        if (v.retired) v.retired += b0;
        if (v.tbox) v.tbox += 2 * b0;
        if (v.bnd) v.bnd += b0;
        if (v.alt_x) { v.alt_x += nx * N * b0; v.alt_u += nu * N * b0; v.alt_T += b0; }
        q.ws = v;
        q.xch.buf = ctx->xch.buf ? ctx->xch.buf + (size_t)2 * MPCMP_XCH_STRIDE * b0 : nullptr;
        q.wx = c.wx ? c.wx + nx * N * b0 : nullptr; q.wu = c.wx ? c.wu + nu * N * b0 : nullptr; q.wT = c.wx ? c.wT + b0 : nullptr;
        q.sx = c.sx ? c.sx + nx * N * b0 : nullptr; q.su = c.su ? c.su + nu * N * b0 : nullptr;
        q.sT = c.sT ? c.sT + b0 : nullptr; q.info = c.info ? c.info + b0 : nullptr;
    }
    return ps;
}
// the further parts' streams start behind the work already on the call's stream (fork) and the call's stream goes on behind them (join); under stream
// capture the events carry the other streams into the graph
static int fork_parts(mpcmp_ctx *ctx, const Parts &ps) {
    if (ps.n > 1) HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ps.p[0].stream));
    for (int h = 1; h < ps.n; h++) HIPCHK(ctx, hipStreamWaitEvent(ps.p[h].stream, ctx->ev_fork, 0));
    return MPCMP_OK;
}
static int join_parts(mpcmp_ctx *ctx, const Parts &ps) {
    for (int h = 1; h < ps.n; h++) { HIPCHK(ctx, hipEventRecord(ctx->ev_join[h - 1], ps.p[h].stream)); HIPCHK(ctx, hipStreamWaitEvent(ps.p[0].stream, ctx->ev_join[h - 1], 0)); }
    return MPCMP_OK;
}

template <int NSEG>
static int solve_impl(mpcmp_ctx *ctx, const SolveCall &c) {
    using D = Dim<NSEG>;
    using S = KSel<NSEG>;
    const S ks(ctx);
    const bool V3C = ks.V3C, V4 = ks.V4, V2 = ks.V2;
    const mpcmp_config cfg = run_config(ctx, c);
    const size_t l_init = InitLds<NSEG>::size * sizeof(double), l_qp = QpLds<S::N1>::size * sizeof(double),
                 l_step = StepLds<NSEG>::size * sizeof(double);
    const size_t l_qp3 = Qp3<S::N3>::sizeL * sizeof(double), l_qp3f = Qp3<S::N3>::sizeF * sizeof(double);
#ifdef MPCMP_WITH_QP4
    const size_t l_qp4 = Qp4<4>::size * sizeof(double);
#endif
    const size_t l_qp2 = Qp2<S::N2>::size * sizeof(double);
    // A large batch is solved as two half-batches on two streams.  Every SQP iteration is a chain of dependent launches
    // (QP -> order -> step), and a QP launch ends in a tail in which most CUs are idle (its problems run 25..700 ADMM
    // iterations, four workgroups per CU); with two independent chains in flight the tail of one half is filled by the other
    // half's next launch.  Replay of the bench workload's iteration counts: -5.8 % makespan.  Results are unaffected (problems
    // are independent); small batches stay on one stream.
    const bool dual = !ctx->single_stream && !c.only_qp && c.B >= 512;      // (also under stream capture: see fork_parts)
    // parts: two; three for the N = 13 kernel from 1024 problems on (round 5, three repeats each: 15.74 - 15.77 k against 15.58 - 15.61 k traj/s on the
    // headline batch; 512 problems — the receding-horizon step — and N = 19 are faster with two: 135.7 k vs 130.0 k re-solves/s, 67.1 k vs 65.2 k traj/s)
    const int parts_auto = (NSEG == 4 && V2 && c.B >= 1024) ? 3 : 2;
    const Parts parts = split(ctx, c, dual ? (ctx->parts_env < 1 ? parts_auto : (ctx->parts_env > 4 ? 4 : ctx->parts_env)) : 1);
    if (int rc = fork_parts(ctx, parts)) return rc;
    for (const Part &p : parts)
        hipLaunchKernelGGL(k_init<NSEG>, dim3(p.B), dim3(D::NT), l_init, p.stream, cfg, p.ws, p.wx, p.wu, p.wT, c.reguess);
    const int iters = c.only_qp ? 1 : cfg.sqp_iters;
    for (int it = 0; it < iters; it++) {
        for (const Part &p : parts) {
            hipEvent_t *ev = (ctx->timing && !c.capturing) ? next_events(ctx) : nullptr;
            if (ev) HIPCHK(ctx, hipEventRecord(ev[0], p.stream));
#ifdef MPCMP_WITH_QP4
            if (V4) {
                WS w3 = p.ws;
                w3.ext_of_int = ctx->d3_ext_of_int; w3.entry_ptr = ctx->d3_entry_ptr; w3.terms = ctx->d3_terms;
                double *fh = ctx->d_fac + (size_t)p.b0 * Qp4Fac<4>::FAC;
                hipLaunchKernelGGL((k_qp3f<4, 1, 4>), dim3(p.B), dim3(1024), Qp3<4>::sizeF * sizeof(double), p.stream, cfg, w3, ctx->d_pat, ctx->xch, p.B, fh);
                hipLaunchKernelGGL((k_qp4<4>), dim3(p.B), dim3(384), l_qp4, p.stream, cfg, w3, (const uint32_t *)ctx->d_lane4, p.B, (const double *)fh);
            }
#else
            if (V4) { ctx->err = "k_qp4 not built"; return MPCMP_EINVAL; }
#endif
            else if (ks.V5) {
                double *fh = ctx->d_fac + (size_t)p.b0 * Qp5Fac<6>::FAC;
                hipLaunchKernelGGL((k_qp3f<6, 1, 5>), dim3(p.B), dim3(1024), Qp3<6>::sizeF * sizeof(double), p.stream, cfg, p.ws, ctx->d_pat, ctx->xch, p.B, fh);
                hipLaunchKernelGGL((k_qp5<6>), dim3(p.B), dim3(768), Qp5<6>::size5 * sizeof(double), p.stream, cfg, p.ws, ctx->d_pat, ctx->xch, p.B, (const double *)fh);
            }
            else if (V3C) {
                WS w3 = p.ws;
                if (NSEG == 4) { w3.ext_of_int = ctx->d3_ext_of_int; w3.entry_ptr = ctx->d3_entry_ptr; w3.terms = ctx->d3_terms; }
                double *fh = ctx->d_fac + (size_t)p.b0 * Qp3<S::N3>::FAC;
                hipLaunchKernelGGL((k_qp3f<S::N3, 1>), dim3(p.B), dim3(1024), l_qp3f, p.stream, cfg, w3, ctx->d_pat, ctx->xch, p.B, fh);
                hipLaunchKernelGGL((k_qp3<S::N3, 1>), dim3(p.B), dim3(512), l_qp3, p.stream, cfg, w3, ctx->d_pat, ctx->xch, p.B, (const double *)fh);
            }
            else if (V2) hipLaunchKernelGGL((k_qp2<S::N2>), dim3(p.B), dim3(1024), l_qp2, p.stream, cfg, p.ws, ctx->streams);
            else hipLaunchKernelGGL((k_qp<S::N1>), dim3(p.B), dim3(Dim<S::N1>::NT), l_qp, p.stream, cfg, p.ws);
            if (ev) HIPCHK(ctx, hipEventRecord(ev[1], p.stream));
            if (c.only_qp) continue;
            hipLaunchKernelGGL(k_step<NSEG>, dim3(p.B), dim3(D::NT), l_step, p.stream, cfg, p.ws, it == iters - 1 ? 1 : 0, it,
                               p.sx, p.su, p.sT, p.info);
        }
    }
    if (int rc = join_parts(ctx, parts)) return rc;
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

template <int NSEG, int NARM>
static int prepare_impl_m(mpcmp_ctx *ctx) {
    using D = DimM<NSEG, NARM>;
    const size_t l_m = D::size * sizeof(double);
    ctx->loop_kernel = "k_qp3";
    if (int rc = set_lds(ctx, k_init_m<NSEG, NARM>, l_m)) return rc;
    if (int rc = set_lds(ctx, k_step_m<NSEG, NARM>, l_m)) return rc;
    if (int rc = set_lds(ctx, k_qp3<NSEG, NARM>, Qp3<NSEG>::sizeL * sizeof(double))) return rc;
    if (int rc = set_lds(ctx, k_qp3f<NSEG, NARM>, Qp3<NSEG>::sizeF * sizeof(double))) return rc;
    return MPCMP_OK;
}

// dynamic-LDS limits of the context's kernels (hipFuncSetAttribute): once per context
static int prepare_kernels(mpcmp_ctx *ctx) {
    if (ctx->narm == 2) return ctx->nseg == 6 ? prepare_impl_m<6, 2>(ctx) : prepare_impl_m<8, 2>(ctx);
    switch (ctx->nseg) {
        case 1: return prepare_impl<1>(ctx);
        case 2: return prepare_impl<2>(ctx);
        case 4: return prepare_impl<4>(ctx);
        case 6: return prepare_impl<6>(ctx);
        case 8: return prepare_impl_m<8, 1>(ctx);
    }
    return MPCMP_EINVAL;
}

// N = 25 and multi-arm OCPs: k_init_m -> K x [k_qp3 (one workgroup per arm), k_step_m]
template <int NSEG, int NARM>
static int solve_impl_m(mpcmp_ctx *ctx, const SolveCall &c) {
    using D = DimM<NSEG, NARM>;
    const mpcmp_config cfg = run_config(ctx, c);
    const size_t l_m = D::size * sizeof(double), l_qp3 = Qp3<NSEG>::sizeL * sizeof(double), l_qp3f = Qp3<NSEG>::sizeF * sizeof(double);
    // two parts on two streams once one part alone fills the chip (one CU per arm): see solve_impl
    const bool dual = !ctx->single_stream && !c.only_qp && c.B * NARM >= 512;
    const Parts parts = split(ctx, c, dual ? 2 : 1);
    if (int rc = fork_parts(ctx, parts)) return rc;
    for (const Part &p : parts)
        hipLaunchKernelGGL((k_init_m<NSEG, NARM>), dim3(p.B), dim3(D::NT), l_m, p.stream, cfg, p.ws.model, p.ws, p.xch, p.wx, p.wu, p.wT, c.reguess);
    const int iters = c.only_qp ? 1 : cfg.sqp_iters;
    for (int it = 0; it < iters; it++) {
        for (const Part &p : parts) {
            hipEvent_t *ev = (ctx->timing && !c.capturing) ? next_events(ctx) : nullptr;
            if (ev) HIPCHK(ctx, hipEventRecord(ev[0], p.stream));
            const int grid = NARM == 1 ? p.B : ((p.B + 7) / 8) * 16;       // arm workgroups of one OCP are 8 apart (k_qp3)
            double *fh = ctx->d_fac + (size_t)p.b0 * NARM * Qp3<NSEG>::FAC;
            hipLaunchKernelGGL((k_qp3f<NSEG, NARM>), dim3(grid), dim3(1024), l_qp3f, p.stream, cfg, p.ws, ctx->d_pat, p.xch, p.B, fh);
            hipLaunchKernelGGL((k_qp3<NSEG, NARM>), dim3(grid), dim3(512), l_qp3, p.stream, cfg, p.ws, ctx->d_pat, p.xch, p.B, (const double *)fh);
            if (ev) HIPCHK(ctx, hipEventRecord(ev[1], p.stream));
            if (c.only_qp) continue;
            hipLaunchKernelGGL((k_step_m<NSEG, NARM>), dim3(p.B), dim3(D::NT), l_m, p.stream, cfg, p.ws.model, p.ws, p.xch,
                               it == iters - 1 ? 1 : 0, it, p.sx, p.su, p.sT, p.info);
        }
    }
    if (int rc = join_parts(ctx, parts)) return rc;
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

static int solve_dispatch(mpcmp_ctx *ctx, const SolveCall &c) {
    if (!ctx) return MPCMP_EINVAL;
    if (c.B < 1) return MPCMP_EINVAL;
    if (c.B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (int rc = c.rh_step ? rows_ok(ctx, c.B, PAYLOAD_ROWS) : solve_rows_ok(ctx, c.B)) return rc;
    if (!c.x0 || !c.xf) return MPCMP_EINVAL;
    if (int rc = warm_all_or_none(ctx, c.wx, c.wu, c.wT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->narm == 2) {
        if (c.only_qp) { ctx->err = "mpcmp_qp_batch is defined for single-arm contexts only"; return MPCMP_EINVAL; }
        if (!c.wx) { ctx->err = "multi-arm solves need a warm start (mpcmp_warm_start_jerk_batch)"; return MPCMP_EINVAL; }
        return ctx->nseg == 6 ? solve_impl_m<6, 2>(ctx, c) : solve_impl_m<8, 2>(ctx, c);
    }
    switch (ctx->nseg) {
        case 1: return solve_impl<1>(ctx, c);
        case 2: return solve_impl<2>(ctx, c);
        case 4: return solve_impl<4>(ctx, c);
        case 6: return solve_impl<6>(ctx, c);
        case 8: return solve_impl_m<8, 1>(ctx, c);
    }
    return MPCMP_EINVAL;
}

// ---- the host-buffer entry points' staging: the context's d_x0 / d_xf / d_w* in, d_s* / d_info (or another triple) out ----
static int upload_problems(mpcmp_ctx *ctx, size_t B, const double *x0, const double *xf, const double *wx, const double *wu, const double *wT, hipStream_t st) {
    const size_t N = ctx->N, nx = ctx->nx, nu = ctx->nu;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_x0, x0, sizeof(double) * nx * B, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_xf, xf, sizeof(double) * nx * B, hipMemcpyHostToDevice, st));
    if (wx) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_wx, wx, sizeof(double) * nx * N * B, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_wu, wu, sizeof(double) * nu * N * B, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_wT, wT, sizeof(double) * B, hipMemcpyHostToDevice, st));
    }
    return MPCMP_OK;
}
// (every host pointer may be NULL: not wanted)
static int download_trajectories(mpcmp_ctx *ctx, size_t B, const double *d_x, const double *d_u, const double *d_T, double *x, double *u, double *T,
                                 mpcmp_info *info, hipStream_t st) {
    const size_t N = ctx->N, nx = ctx->nx, nu = ctx->nu;
    if (x) HIPCHK(ctx, hipMemcpyAsync(x, d_x, sizeof(double) * nx * N * B, hipMemcpyDeviceToHost, st));
    if (u) HIPCHK(ctx, hipMemcpyAsync(u, d_u, sizeof(double) * nu * N * B, hipMemcpyDeviceToHost, st));
    if (T) HIPCHK(ctx, hipMemcpyAsync(T, d_T, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (info) HIPCHK(ctx, hipMemcpyAsync(info, ctx->d_info, sizeof(mpcmp_info) * B, hipMemcpyDeviceToHost, st));
    return MPCMP_OK;
}
// the solve of the staged problems into the staged outputs; warm: with the staged start guess
static SolveCall staged_call(const mpcmp_ctx *ctx, int B, bool warm, hipStream_t st) {
    SolveCall c;
    c.B = B; c.x0 = ctx->d_x0; c.xf = ctx->d_xf;
    if (warm) { c.wx = ctx->d_wx; c.wu = ctx->d_wu; c.wT = ctx->d_wT; }
    c.sx = ctx->d_sx; c.su = ctx->d_su; c.sT = ctx->d_sT; c.info = ctx->d_info; c.stream = st;
    return c;
}

extern "C" int mpcmp_solve_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf,
                                        const double *d_wx, const double *d_wu, const double *d_wT, double *d_sx,
                                        double *d_su, double *d_sT, mpcmp_info *d_info, void *hip_stream) {
    if (!d_sx || !d_su || !d_sT) return MPCMP_EINVAL;
    return solve_dispatch(ctx, SolveCall{B, d_x0, d_xf, d_wx, d_wu, d_wT, d_sx, d_su, d_sT, d_info, (hipStream_t)hip_stream});
}

extern "C" int mpcmp_solve_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *wx,
                                 const double *wu, const double *wT, double *sx, double *su, double *sT, mpcmp_info *info) {
    if (!ctx || !x0 || !xf || !sx || !su || !sT) return MPCMP_EINVAL;
    if (B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (int rc = solve_rows_ok(ctx, B)) return rc;
    if (int rc = warm_all_or_none(ctx, wx, wu, wT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = upload_problems(ctx, B, x0, xf, wx, wu, wT, st)) return rc;
    if (int rc = solve_dispatch(ctx, staged_call(ctx, B, wx != nullptr, st))) return rc;
    if (int rc = download_trajectories(ctx, B, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

#define SINGLE_ARM_ONLY(ctx) do { if ((ctx)->narm != 1) { (ctx)->err = "this entry point is defined for single-arm contexts only"; return MPCMP_EINVAL; } } while (0)

extern "C" int mpcmp_warm_start_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, double *wx, double *wu, double *wT) {
    if (!ctx || !x0 || !xf || !wx || !wu || !wT || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    if (int rc = rows_ok(ctx, B, TIME_ROWS)) return rc;
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = ctx->N, n = ctx->n;
    hipStream_t st = ctx->stream;
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    // k_init alone: the built-in initialiser writes the iterate z = [xs|us|T]
    const SolveCall plain;
    const mpcmp_config save = run_config(ctx, plain);
    WS w = ctx->ws; w.x0 = ctx->d_x0; w.xf = ctx->d_xf; w.tbox = run_rows(ctx, plain); w.bnd = run_bounds(ctx, plain);
#define LAUNCH_INIT(NS) { const size_t l = InitLds<NS>::size * sizeof(double); \
        hipLaunchKernelGGL(k_init<NS>, dim3(B), dim3(Dim<NS>::NT), l, st, save, w, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, 0); }
    switch (ctx->nseg) { case 1: LAUNCH_INIT(1) break; case 2: LAUNCH_INIT(2) break; case 4: LAUNCH_INIT(4) break; case 6: LAUNCH_INIT(6) break;
        case 8: { const size_t l = DimM<8, 1>::size * sizeof(double);
                  hipLaunchKernelGGL((k_init_m<8, 1>), dim3(B), dim3(512), l, st, save, ctx->d_model, w, ctx->xch, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, 0); } break; }
#undef LAUNCH_INIT
    HIPCHK(ctx, hipGetLastError());
    std::vector<double> z((size_t)B * n);
    HIPCHK(ctx, hipMemcpyAsync(z.data(), ctx->ws.z, sizeof(double) * n * B, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int b = 0; b < B; b++) {
        std::memcpy(wx + (size_t)b * 14 * N, z.data() + (size_t)b * n, sizeof(double) * 14 * N);
        std::memcpy(wu + (size_t)b * 7 * N, z.data() + (size_t)b * n + 14 * N, sizeof(double) * 7 * N);
        wT[b] = z[(size_t)b * n + 21 * N];
    }
    return MPCMP_OK;
}

// Device staging of the host-pointer entry points, in the context's scratch: owned by the context and only ever grown, so that after the first call
// of a given size these entry points do not allocate (a control loop calls get_MPC_point / get_RK_point every tick).
// An entry point DECLARES every device array it needs, each with the variable that will hold its device pointer, an element count and what happens to
// it: in() is copied from a host pointer by upload(), out() is copied to one by finish(), inout() both.  upload() adds up the aligned sizes, grows the
// scratch at most once and only then fills the variables in, so no pointer exists that a growth could leave dangling.  A NULL host pointer is an array
// the caller did not give: its device pointer stays NULL, and nothing is reserved or copied for it.
struct Stage {
    explicit Stage(mpcmp_ctx *c) : ctx(c) {}
    template <typename T> void in(T **dev, const T *host, size_t count) { *dev = nullptr; add(dev, host, nullptr, count * sizeof(T)); }
    template <typename T> void out(T **dev, T *host, size_t count) { *dev = nullptr; add(dev, nullptr, host, count * sizeof(T)); }
    template <typename T> void inout(T **dev, T *host, size_t count) { *dev = nullptr; add(dev, host, host, count * sizeof(T)); }
    // after the last declaration, before the launch: the scratch, the device pointers, and every input copy on ctx->stream
    int upload() {
        size_t total = 0;
        for (int i = 0; i < n; i++) total += aligned(items[i].bytes);
        if (total > ctx->scratch_bytes) {
            if (ctx->scratch) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->scratch); ctx->scratch = nullptr; ctx->scratch_bytes = 0; }
            const size_t want = total < (1u << 20) ? (1u << 20) : total;
            if (hipMalloc(&ctx->scratch, want) != hipSuccess) { ctx->scratch = nullptr; ctx->err = "device scratch allocation failed"; return MPCMP_ERUNTIME; }
            ctx->scratch_bytes = want;
        }
        char *p = static_cast<char *>(ctx->scratch);
        for (int i = 0; i < n; i++) {
            items[i].dev = p;
            std::memcpy(items[i].var, &p, sizeof p);      // (the variables are pointers of several types: no cast of one to the other's address)
            p += aligned(items[i].bytes);
        }
        for (int i = 0; i < n; i++)
            if (items[i].src) HIPCHK(ctx, hipMemcpyAsync(items[i].dev, items[i].src, items[i].bytes, hipMemcpyHostToDevice, ctx->stream));
        return MPCMP_OK;
    }
    // after the launch: every output copy on ctx->stream, and the wait for it
    int finish() {
        for (int i = 0; i < n; i++)
            if (items[i].dst) HIPCHK(ctx, hipMemcpyAsync(items[i].dst, items[i].dev, items[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return MPCMP_OK;
    }

private:
    struct Item { void *var, *dev; const void *src; void *dst; size_t bytes; };
    static constexpr int MAX_ITEMS = 12;
    static size_t aligned(size_t bytes) { return (bytes + 255) / 256 * 256; }
    void add(void *var, const void *src, void *dst, size_t bytes) {
        if (!src && !dst) return;
        assert(n < MAX_ITEMS);
        items[n++] = {var, nullptr, src, dst, bytes};
    }
    mpcmp_ctx *ctx;
    Item items[MAX_ITEMS];
    int n = 0;
};

// ---- time scaling and the time-synchronised solve (time_sync.hpp) ----
static int time_scale_enqueue(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_sx, const double *d_su, const double *d_sT,
                              const double *d_Tn, const int *d_skip, double *d_ox, double *d_ou, double *d_oT, hipStream_t st) {
    hipLaunchKernelGGL(k_time_scale, dim3(B), dim3(256), 0, st, ctx->N, ctx->narm, d_x0, d_xf, d_sx, d_su, d_sT, d_Tn, d_skip, d_ox, d_ou, d_oT);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_time_scale_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_sx, const double *d_su,
                                             const double *d_sT, const double *d_Tn, double *d_ox, double *d_ou, double *d_oT, void *hip_stream) {
    if (!ctx || B < 1 || !d_x0 || !d_xf || !d_sx || !d_su || !d_sT || !d_Tn || !d_ox || !d_ou || !d_oT) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return time_scale_enqueue(ctx, B, d_x0, d_xf, d_sx, d_su, d_sT, d_Tn, nullptr, d_ox, d_ou, d_oT, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_time_scale_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *sx, const double *su, const double *sT,
                                      const double *Tn, double *ox, double *ou, double *oT) {
    if (!ctx || B < 1 || !x0 || !xf || !sx || !su || !sT || !Tn || !ox || !ou || !oT) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, nx = ctx->nx * nb, nxN = nx * ctx->N, nuN = ctx->nu * nb * ctx->N;
    Stage sg(ctx);
    double *d0, *d1, *dx, *du, *dT, *dn, *qx, *qu, *qT;
    sg.in(&d0, x0, nx); sg.in(&d1, xf, nx); sg.in(&dx, sx, nxN); sg.in(&du, su, nuN); sg.in(&dT, sT, nb); sg.in(&dn, Tn, nb);
    sg.out(&qx, ox, nxN); sg.out(&qu, ou, nuN); sg.out(&qT, oT, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = time_scale_enqueue(ctx, B, d0, d1, dx, du, dT, dn, nullptr, qx, qu, qT, ctx->stream)) return rc;
    return sg.finish();
}

static int synced_check(mpcmp_ctx *ctx, int B, int n_groups, const double *wx, const double *wu, const double *wT) {
    if (B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (n_groups < 0 || n_groups > ctx->max_batch) { ctx->err = "mpcmp_solve_batch_synced: n_groups must be in [0, max_batch]"; return MPCMP_EINVAL; }
    if (int rc = warm_all_or_none(ctx, wx, wu, wT)) return rc;
    if (int rc = solve_rows_ok(ctx, B)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_sg_count) {            // first use
        const size_t M = ctx->max_batch, N = ctx->N;
        if (int rc = dalloc(ctx, &ctx->d_sg_count, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_skip, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_status, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_key, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_T, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_rows, 2 * M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_Tn, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_wx, M * ctx->nx * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_wu, M * ctx->nu * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_wT, M)) return rc;
    }
    return MPCMP_OK;
}

// pass 1 (the call as given), the group times, the pass-2 mask / rows / start guess, pass 2: all on the call's stream, no host round trip
static int synced_enqueue(mpcmp_ctx *ctx, const SolveCall &pass1, const int *d_group, int n_groups, double *d_gT) {
    const int B = pass1.B;
    hipStream_t st = pass1.stream;
    if (int rc = solve_dispatch(ctx, pass1)) return rc;
    const int G = n_groups > 0 ? n_groups : 1;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_sg_key, 0, sizeof(unsigned long long) * G, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_sg_count, 0, sizeof(int) * G, st));
    hipLaunchKernelGGL(k_sync_tmax, dim3((B + 255) / 256), dim3(256), 0, st, B, d_group, n_groups, (const int *)ctx->ws.status, (const double *)pass1.sT,
                       ctx->d_sg_key, ctx->d_sg_count);
    const int np = B > n_groups ? B : n_groups;
    hipLaunchKernelGGL(k_sync_prepare, dim3((np + 255) / 256), dim3(256), 0, st, B, d_group, n_groups, (const int *)ctx->ws.status, (const double *)pass1.sT,
                       (const unsigned long long *)ctx->d_sg_key, (const int *)ctx->d_sg_count, d_gT, ctx->d_sg_skip, ctx->d_sg_rows, ctx->d_sg_Tn,
                       ctx->d_sg_status);
    HIPCHK(ctx, hipGetLastError());
    if (int rc = time_scale_enqueue(ctx, B, pass1.x0, pass1.xf, pass1.sx, pass1.su, pass1.sT, ctx->d_sg_Tn, ctx->d_sg_skip, ctx->d_sg_wx, ctx->d_sg_wu, ctx->d_sg_wT, st))
        return rc;
    // pass 2: every slot is launched; the ones not re-solved return at once (WS::retired) and keep their pass-1 outputs
    SolveCall pass2 = pass1;
    pass2.wx = ctx->d_sg_wx; pass2.wu = ctx->d_sg_wu; pass2.wT = ctx->d_sg_wT;
    pass2.tw_rows = ctx->d_sg_rows; pass2.skip = ctx->d_sg_skip;
    if (int rc = solve_dispatch(ctx, pass2)) return rc;
    // (at N = 25 the skipped slots' QP kernels ran in pass 2 and added to their status words: the next solve sees pass 1's, as after a plain solve)
    hipLaunchKernelGGL(k_sync_restore, dim3((B + 255) / 256), dim3(256), 0, st, B, (const int *)ctx->d_sg_skip, (const int *)ctx->d_sg_status,
                       ctx->ws.status);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_solve_batch_synced_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_wx, const double *d_wu,
                                               const double *d_wT, const int *d_group, int n_groups, double *d_sx, double *d_su, double *d_sT,
                                               mpcmp_info *d_info, double *d_group_T, void *hip_stream) {
    if (!ctx || !d_x0 || !d_xf || !d_group || !d_sx || !d_su || !d_sT) return MPCMP_EINVAL;
    if (int rc = synced_check(ctx, B, n_groups, d_wx, d_wu, d_wT)) return rc;
    return synced_enqueue(ctx, SolveCall{B, d_x0, d_xf, d_wx, d_wu, d_wT, d_sx, d_su, d_sT, d_info, (hipStream_t)hip_stream}, d_group, n_groups,
                          d_group_T ? d_group_T : ctx->d_sg_T);
}

extern "C" int mpcmp_solve_batch_synced(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *wx, const double *wu, const double *wT,
                                        const int *group, int n_groups, double *sx, double *su, double *sT, mpcmp_info *info, double *group_T) {
    if (!ctx || !x0 || !xf || !group || !sx || !su || !sT) return MPCMP_EINVAL;
    if (int rc = synced_check(ctx, B, n_groups, wx, wu, wT)) return rc;
    for (int i = 0; i < B; i++)
        if (group[i] < -1 || group[i] >= n_groups) {
            ctx->err = "mpcmp_solve_batch_synced: group[" + std::to_string(i) + "] must be -1 or in [0, n_groups)"; return MPCMP_EINVAL;
        }
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    int *dg;
    sg.in(&dg, group, B);
    if (int rc = upload_problems(ctx, B, x0, xf, wx, wu, wT, st)) return rc;
    if (int rc = sg.upload()) return rc;
    if (int rc = synced_enqueue(ctx, staged_call(ctx, B, wx != nullptr, st), dg, n_groups, ctx->d_sg_T)) return rc;
    if (int rc = download_trajectories(ctx, B, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    if (group_T && n_groups > 0) HIPCHK(ctx, hipMemcpyAsync(group_T, ctx->d_sg_T, sizeof(double) * n_groups, hipMemcpyDeviceToHost, st));
    return sg.finish();
}

// ---- jerk-limited, time-synchronised warm start / comparison trajectory (stands in for Ruckig) ----
// vmax / amax: NULL = the context's margin-applied bounds (the *_lim_* entry points pass a caller's own: ruckig::InputParameter::max_velocity / max_acceleration)
static int jerk_limits(mpcmp_ctx *ctx, const double *vmax, const double *amax, const double *jmax, JerkLimits &lim) {
    for (int j = 0; j < 7; j++) {
        lim.v[j] = vmax ? vmax[j] : ctx->cfg.ubx[7 + j]; lim.a[j] = amax ? amax[j] : ctx->cfg.ubu[j]; lim.j[j] = jmax[j];
        if (!(lim.v[j] > 0.0) || !(lim.a[j] > 0.0) || !(lim.j[j] > 0.0)) { ctx->err = "velocity, acceleration and jerk limits must be positive"; return MPCMP_EINVAL; }
    }
    return MPCMP_OK;
}

// boundary accelerations d_acc0 / d_accT: device [B][7], either may be NULL (= zero); single-arm contexts only (a multi-arm warm start has none)
static int warm_start_jerk_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_acc0, const double *d_accT,
                                  const double *vmax, const double *amax, const double *jmax, double *d_wx, double *d_wu, double *d_wT, void *hip_stream,
                                  const int *need_status = nullptr, int need_mask = 0) {
    if (!ctx || !d_x0 || !d_xf || !jmax || !d_wx || !d_wu || !d_wT || B < 1) return MPCMP_EINVAL;
    if ((d_acc0 || d_accT) && ctx->narm != 1) { ctx->err = "boundary accelerations: single-arm contexts only"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JerkLimits lim;
    if (int rc = jerk_limits(ctx, vmax, amax, jmax, lim)) return rc;
    if (ctx->narm == 2) {
        // per-arm generator on B * narm arm problems, then the merge to the common (slowest arm's) duration: multi_kernels.hpp
        if (B > ctx->max_batch) return MPCMP_ETOOBIG;
        hipStream_t s2 = (hipStream_t)hip_stream;
        const int cnt = B * 2 * 14;
        hipLaunchKernelGGL((k_split_states<2>), dim3((cnt + 255) / 256), dim3(256), 0, s2, B, d_x0, ctx->d_ax0);
        hipLaunchKernelGGL((k_split_states<2>), dim3((cnt + 255) / 256), dim3(256), 0, s2, B, d_xf, ctx->d_axf);
        hipLaunchKernelGGL(k_warm_jerk, dim3(B * 2), dim3(64), 0, s2, ctx->nseg, lim, ctx->d_ax0, ctx->d_axf, (const double *)nullptr, (const double *)nullptr, ctx->d_awx, ctx->d_awu, ctx->d_awT,
                           need_status, need_mask, 2);
        hipLaunchKernelGGL((k_warm_merge<2>), dim3(B), dim3(256), 0, s2, ctx->N, B, ctx->d_awx, ctx->d_awu, ctx->d_awT, d_x0, d_xf, d_wx, d_wu, d_wT);
        HIPCHK(ctx, hipGetLastError());
        return MPCMP_OK;
    }
    // the stream exactly as given (NULL = the legacy default stream), like the other *_device entry points: the solve that
    // consumes the warm start is enqueued on the same stream and is ordered behind this launch
    hipLaunchKernelGGL(k_warm_jerk, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, ctx->nseg, lim, d_x0, d_xf, d_acc0, d_accT, d_wx, d_wu, d_wT, need_status, need_mask, 1);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}
extern "C" int mpcmp_warm_start_jerk_acc_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_acc0, const double *d_accT,
                                                      const double *jmax, double *d_wx, double *d_wu, double *d_wT, void *hip_stream) {
    return warm_start_jerk_device(ctx, B, d_x0, d_xf, d_acc0, d_accT, nullptr, nullptr, jmax, d_wx, d_wu, d_wT, hip_stream);
}
extern "C" int mpcmp_warm_start_jerk_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *jmax,
                                                  double *d_wx, double *d_wu, double *d_wT, void *hip_stream) {
    return mpcmp_warm_start_jerk_acc_batch_device(ctx, B, d_x0, d_xf, nullptr, nullptr, jmax, d_wx, d_wu, d_wT, hip_stream);
}

// Boundary states the generator cannot honour: the acceleration limit yields to a boundary acceleration above it (include/mpcmp.h), but an
// acceleration that cannot be brought to zero inside the VELOCITY limit — |v0 + a0 |a0| / 2J| > V at the start, |vT - aT |aT| / 2J| > V at the target —
// would overshoot the state box of the OCP: MPCMP_EINVAL, as Ruckig rejects such an input (ErrorInvalidInput; the shim's otg.calculate returns it).
// Host-pointer entry points only: the *_device variants never read their inputs on the host.
static int check_boundary_acc(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                              const double *vmax, const double *jmax) {
    if ((!acc0 && !accT) || ctx->narm != 1) return MPCMP_OK;
    for (int b = 0; b < B; b++)
        for (int j = 0; j < 7; j++) {
            const double V = (vmax ? vmax[j] : ctx->cfg.ubx[7 + j]) * (1.0 + 1e-9), J = jmax[j];
            if (!(J > 0.0)) continue;      // (reported by jerk_limits)
            const double a0 = acc0 ? acc0[7 * b + j] : 0.0, aT = accT ? accT[7 * b + j] : 0.0;
            const double v0 = x0[14 * b + 7 + j], vT = xf[14 * b + 7 + j];
            const double va = v0 + a0 * std::fabs(a0) / (2.0 * J), vb = vT - aT * std::fabs(aT) / (2.0 * J);
            // (a boundary VELOCITY outside the limit is the caller's business, as before: that joint falls back to the quintic of the common duration)
            if ((std::fabs(v0) <= V && std::fabs(va) > V) || (std::fabs(vT) <= V && std::fabs(vb) > V)) {
                std::ostringstream os;
                os << "problem " << b << ", joint " << j << ": the boundary acceleration cannot be brought to zero inside the velocity limit";
                ctx->err = os.str();
                return MPCMP_EINVAL;
            }
        }
    return MPCMP_OK;
}

extern "C" int mpcmp_warm_start_jerk_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *vmax, const double *amax, const double *jmax, double *wx, double *wu, double *wT) {
    if (!ctx || !x0 || !xf || !jmax || !wx || !wu || !wT || B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = check_boundary_acc(ctx, B, x0, xf, acc0, accT, vmax, jmax)) return rc;
    if ((acc0 || accT) && ctx->narm != 1) { ctx->err = "boundary accelerations: single-arm contexts only"; return MPCMP_EINVAL; }
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *da0, *daT;
    sg.in(&da0, acc0, 7 * (size_t)B); sg.in(&daT, accT, 7 * (size_t)B);
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = sg.upload()) return rc;
    if (int rc = warm_start_jerk_device(ctx, B, ctx->d_x0, ctx->d_xf, da0, daT, vmax, amax, jmax, ctx->d_wx, ctx->d_wu, ctx->d_wT, st)) return rc;
    if (int rc = download_trajectories(ctx, B, ctx->d_wx, ctx->d_wu, ctx->d_wT, wx, wu, wT, nullptr, st)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_warm_start_jerk_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *jmax, double *wx, double *wu, double *wT) {
    return mpcmp_warm_start_jerk_lim_batch(ctx, B, x0, xf, acc0, accT, nullptr, nullptr, jmax, wx, wu, wT);
}
extern "C" int mpcmp_warm_start_jerk_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax,
                                           double *wx, double *wu, double *wT) {
    return mpcmp_warm_start_jerk_acc_batch(ctx, B, x0, xf, nullptr, nullptr, jmax, wx, wu, wT);
}

extern "C" int mpcmp_jerk_trajectory_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *vmax, const double *amax, const double *jmax, int n_pts, double *out, double *T_out) {
    if (!ctx || !x0 || !xf || !jmax || !out || B < 1 || n_pts < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JerkLimits lim;
    if (int rc = jerk_limits(ctx, vmax, amax, jmax, lim)) return rc;
    if (int rc = check_boundary_acc(ctx, B, x0, xf, acc0, accT, vmax, jmax)) return rc;
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *da0, *daT, *dout;
    sg.in(&da0, acc0, 7 * (size_t)B); sg.in(&daT, accT, 7 * (size_t)B); sg.out(&dout, out, (size_t)B * (n_pts + 1) * 22);
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = sg.upload()) return rc;
    hipLaunchKernelGGL(k_jerk_traj, dim3(B), dim3(64), 0, st, lim, ctx->d_x0, ctx->d_xf, da0, daT, n_pts, dout, ctx->d_wT);
    HIPCHK(ctx, hipGetLastError());
    if (T_out) HIPCHK(ctx, hipMemcpyAsync(T_out, ctx->d_wT, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    return sg.finish();
}

extern "C" int mpcmp_jerk_trajectory_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *jmax, int n_pts, double *out, double *T_out) {
    return mpcmp_jerk_trajectory_lim_batch(ctx, B, x0, xf, acc0, accT, nullptr, nullptr, jmax, n_pts, out, T_out);
}
extern "C" int mpcmp_jerk_trajectory_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax, int n_pts,
                                           double *out, double *T_out) {
    return mpcmp_jerk_trajectory_acc_batch(ctx, B, x0, xf, nullptr, nullptr, jmax, n_pts, out, T_out);
}

// MotionPlanner::get_RK_point (motionPlanner.hpp:130-142)
extern "C" int mpcmp_jerk_point_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                          const double *vmax, const double *amax, const double *jmax, const double *time, double *out, double *T_out) {
    if (!ctx || !x0 || !xf || !jmax || !time || !out || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JerkLimits lim;
    if (int rc = jerk_limits(ctx, vmax, amax, jmax, lim)) return rc;
    if (int rc = check_boundary_acc(ctx, B, x0, xf, acc0, accT, vmax, jmax)) return rc;
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *dt, *da0, *daT, *dout;
    sg.in(&dt, time, B); sg.in(&da0, acc0, 7 * (size_t)B); sg.in(&daT, accT, 7 * (size_t)B); sg.out(&dout, out, 28 * (size_t)B);
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = sg.upload()) return rc;
    hipLaunchKernelGGL(k_jerk_point, dim3(B), dim3(64), 0, st, ctx->d_model, lim, ctx->d_x0, ctx->d_xf, da0, daT, dt, dout, ctx->d_wT);
    HIPCHK(ctx, hipGetLastError());
    if (T_out) HIPCHK(ctx, hipMemcpyAsync(T_out, ctx->d_wT, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    return sg.finish();
}

extern "C" int mpcmp_jerk_point_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                          const double *jmax, const double *time, double *out, double *T_out) {
    return mpcmp_jerk_point_lim_batch(ctx, B, x0, xf, acc0, accT, nullptr, nullptr, jmax, time, out, T_out);
}
extern "C" int mpcmp_jerk_point_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax, const double *time,
                                      double *out, double *T_out) {
    return mpcmp_jerk_point_acc_batch(ctx, B, x0, xf, nullptr, nullptr, jmax, time, out, T_out);
}

// MotionPlanner::get_MPC_point (motionPlanner.hpp:118-128)
extern "C" int mpcmp_mpc_point_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, const double *time,
                                     double *out) {
    if (!ctx || !sx || !su || !sT || !time || !out || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dt, *dout;
    sg.in(&dx, sx, 14 * NB); sg.in(&du, su, 7 * NB); sg.in(&dT, sT, nb); sg.in(&dt, time, nb); sg.out(&dout, out, 28 * nb);
    if (int rc = sg.upload()) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_mpc_point, dim3((B + 63) / 64), dim3(64), 0, ctx->stream, md, ms, ctx->nseg, B, dx, du, dT, dt, dout);
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

extern "C" int mpcmp_qp_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *xs,
                              const double *us, const double *T, double *p, double *y, int *iters) {
    if (!ctx || !x0 || !xf || !xs || !us || !T || !p || !y || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    if (int rc = solve_rows_ok(ctx, B)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = upload_problems(ctx, B, x0, xf, xs, us, T, st)) return rc;
    SolveCall c = staged_call(ctx, B, true, st);
    c.info = nullptr; c.only_qp = 1;
    if (int rc = solve_dispatch(ctx, c)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(p, ctx->ws.p, sizeof(double) * ctx->n * B, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(y, ctx->ws.y, sizeof(double) * ctx->mn * B, hipMemcpyDeviceToHost, st));
    if (iters) HIPCHK(ctx, hipMemcpyAsync(iters, ctx->ws.qpit, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// leaf kernels
extern "C" int mpcmp_rnea_batch(mpcmp_ctx *ctx, int n, const double *q, const double *qd, const double *qdd, double *tau) {
    if (!ctx || n < 1 || !q || !qd || !qdd || !tau) return MPCMP_EINVAL;
    if (int rc = rows_ok(ctx, n, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n7 = 7 * (size_t)n;
    Stage sg(ctx);
    double *dq, *dv, *da, *dt;
    sg.in(&dq, q, n7); sg.in(&dv, qd, n7); sg.in(&da, qdd, n7); sg.out(&dt, tau, n7);
    if (int rc = sg.upload()) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_rnea_batch, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, md, ms, n, dq, dv, da, dt);
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

extern "C" int mpcmp_eval_constraints_batch(mpcmp_ctx *ctx, int n, const double *x, const double *u, double *g, double *G) {
    if (!ctx || n < 1 || !x || !u || !g || !G) return MPCMP_EINVAL;
    if (int rc = rows_ok(ctx, n, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t np = n;
    Stage sg(ctx);
    double *dx, *du, *dg, *dG;
    sg.in(&dx, x, 14 * np); sg.in(&du, u, 7 * np); sg.out(&dg, g, 8 * np); sg.out(&dG, G, 176 * np);
    if (int rc = sg.upload()) return rc;
    constexpr int NS = 4;
    const size_t l = EvalLds<NS>::size * sizeof(double);
    if (int rc = set_lds(ctx, k_eval_constraints<NS>, l)) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    const int per = ms ? 1 : Dim<NS>::N;           // points per workgroup: one with per-point models (k_eval_constraints)
    hipLaunchKernelGGL(k_eval_constraints<NS>, dim3((n + per - 1) / per), dim3(Dim<NS>::NT), l, ctx->stream, ctx->cfg, md, ms, n, dx, du, dg, dG);
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

extern "C" int mpcmp_sample_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT,
                                         int n_pts, double *d_out, void *hip_stream) {
    if (!ctx || B < 1 || n_pts < 1 || !d_sx || !d_su || !d_sT || !d_out) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long total = (long)B * (n_pts + 1);
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_sample, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, (hipStream_t)hip_stream, md, ms,
                       ctx->nseg, B, n_pts, d_sx, d_su, d_sT, d_out);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_sample_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_pts, double *out) {
    if (!ctx || B < 1 || n_pts < 1 || !sx || !su || !sT || !out) return MPCMP_EINVAL;
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dout;
    sg.in(&dx, sx, 14 * NB); sg.in(&du, su, 7 * NB); sg.in(&dT, sT, nb); sg.out(&dout, out, nb * (n_pts + 1) * 29);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sample_batch_device(ctx, B, dx, du, dT, n_pts, dout, ctx->stream)) return rc;
    return sg.finish();
}


// examples/benchmark.cpp:58-160 for a batch of trajectories (either the initial guess or the MPC solution)
extern "C" int mpcmp_traj_stats_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, const double *xf,
                                      int n_pts, double *out) {
    if (!ctx || B < 1 || n_pts < 1 || !sx || !su || !sT || !xf || !out) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    // the kernel keeps the n_pts+1 samples of one trajectory (28 doubles each) in LDS: 160 KB per workgroup on gfx950
    if (sizeof(double) * 28 * (size_t)(n_pts + 1) > 150 * 1024) { ctx->err = "mpcmp_traj_stats_batch: n_pts must be <= 684 (the samples of one trajectory are held in LDS)"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double jerk[7], j10[7];
    mpcmp_default_limits(nullptr, nullptr, nullptr, nullptr, jerk, nullptr);
    for (int r = 0; r < 7; r++) j10[r] = 10.0 * jerk[r];                     // benchmark.cpp:128
    const size_t nb = B, NB = ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *df, *dj, *dout;
    sg.in(&dx, sx, 14 * NB); sg.in(&du, su, 7 * NB); sg.in(&dT, sT, nb); sg.in(&df, xf, 14 * nb); sg.in(&dj, j10, 7); sg.out(&dout, out, 74 * nb);
    if (int rc = sg.upload()) return rc;
    const size_t lds = sizeof(double) * 28 * (size_t)(n_pts + 1);
    if (int rc = set_lds(ctx, k_traj_stats, lds)) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_traj_stats, dim3(B), dim3(256), lds, ctx->stream, md, ms, ctx->nseg, n_pts, dx, du, dT, df, 1.7, 2.5, dj, dout);   // pandaWrapper.hpp:37-38
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// clearance checks (clearance.hpp; the kernels are in clearance.hip)
extern "C" int mpcmp_set_robot_spheres(mpcmp_ctx *ctx, int arm, int n, const mpcmp_sphere *sp) {
    if (!ctx) { g_err = "mpcmp_set_robot_spheres: no context"; return MPCMP_EINVAL; }
    if (arm < 0 || arm >= ctx->narm || n < 0 || n > CLR_MAX_SPH || (n > 0 && !sp)) {
        ctx->err = "mpcmp_set_robot_spheres: arm must be in [0, narm) and n in [0, 64] with the spheres given"; return MPCMP_EINVAL;
    }
    for (int i = 0; i < n; i++) {
        const mpcmp_sphere &s = sp[i];
        if (s.joint < 0 || s.joint > 6 || !std::isfinite(s.c[0]) || !std::isfinite(s.c[1]) || !std::isfinite(s.c[2]) || !std::isfinite(s.r) || !(s.r > 0.0)) {
            ctx->err = "mpcmp_set_robot_spheres: sphere " + std::to_string(i) + ": joint in 0..6, finite centre and r > 0 required"; return MPCMP_EINVAL;
        }
    }
    int cnt[2] = {ctx->clr_nsph[0], ctx->clr_nsph[1]};
    cnt[arm] = n;
    ClrSphere tab[2 * CLR_MAX_SPH];
    int k = 0;
    for (int a = 0; a < ctx->narm; a++)
        for (int i = 0; i < cnt[a]; i++, k++) {
            const mpcmp_sphere &s = a == arm ? sp[i] : ctx->clr_sph[a][i];
            tab[k].c[0] = s.c[0]; tab[k].c[1] = s.c[1]; tab[k].c[2] = s.c[2]; tab[k].r = s.r; tab[k].joint = s.joint; tab[k].arm = a;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());          // (checks may be in flight on any stream of the caller: they read this table)
    if (k > 0) HIPCHK(ctx, hipMemcpy(ctx->d_clr_sph, tab, sizeof(ClrSphere) * k, hipMemcpyHostToDevice));
    for (int i = 0; i < n; i++) ctx->clr_sph[arm][i] = sp[i];
    ctx->clr_nsph[arm] = n;
    return MPCMP_OK;
}

static int obstacles_check(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *obs) {
    if (!ctx) { g_err = "mpcmp_set_obstacles: no context"; return MPCMP_EINVAL; }
    if (n_sets < 0 || n_sets > ctx->max_batch || n_obs < 0 || n_obs > CLR_MAX_OBS || (n_sets > 0 && n_obs > 0 && !obs)) {
        ctx->err = "mpcmp_set_obstacles: n_sets must be in [0, max_batch] and n_obs in [0, 256] with the obstacles given"; return MPCMP_EINVAL;
    }
    const size_t want = (size_t)n_sets * n_obs;
    if (want > ctx->clr_obs_cap) {          // grow: later launches read the new buffer; wait for the ones that read the old one
        HIPCHK(ctx, hipSetDevice(ctx->device));
        void *q = nullptr;
        HIPCHK(ctx, hipMalloc(&q, want * sizeof(mpcmp_obstacle)));
        if (ctx->d_clr_obs) {
            HIPCHK(ctx, hipDeviceSynchronize());
            ctx->allocs.erase(std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *)ctx->d_clr_obs));
            (void)hipFree(ctx->d_clr_obs);
        }
        ctx->allocs.push_back(q); ctx->d_clr_obs = (mpcmp_obstacle *)q; ctx->clr_obs_cap = want;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_set_obstacles(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *obs) {
    if (ctx && n_sets > 0 && n_sets <= ctx->max_batch && n_obs > 0 && n_obs <= CLR_MAX_OBS && obs)
        for (size_t i = 0; i < (size_t)n_sets * n_obs; i++) {
            const mpcmp_obstacle &o = obs[i];
            bool ok = o.type >= MPCMP_OBS_SPHERE && o.type <= MPCMP_OBS_HALFSPACE && std::isfinite(o.r);
            for (int d = 0; d < 3 && ok; d++) ok = std::isfinite(o.a[d]) && std::isfinite(o.b[d]);
            if (ok && o.type != MPCMP_OBS_HALFSPACE) ok = o.r >= 0.0;
            if (ok && o.type == MPCMP_OBS_BOX) ok = o.b[0] > 0.0 && o.b[1] > 0.0 && o.b[2] > 0.0;
            if (ok && o.type == MPCMP_OBS_HALFSPACE) ok = std::fabs(std::sqrt(o.a[0] * o.a[0] + o.a[1] * o.a[1] + o.a[2] * o.a[2]) - 1.0) <= 1e-9;
            if (!ok) {
                ctx->err = "mpcmp_set_obstacles: set " + std::to_string(i / n_obs) + ", obstacle " + std::to_string(i % n_obs) +
                           ": known type, finite values, r >= 0, box half extents > 0 and a unit half-space normal required";
                return MPCMP_EINVAL;
            }
        }
    if (int rc = obstacles_check(ctx, n_sets, n_obs, obs)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());          // (checks may be in flight on any stream of the caller: they read these sets)
    if (n_sets > 0 && n_obs > 0) HIPCHK(ctx, hipMemcpy(ctx->d_clr_obs, obs, sizeof(mpcmp_obstacle) * n_sets * n_obs, hipMemcpyHostToDevice));
    ctx->clr_sets = n_obs > 0 ? n_sets : 0; ctx->clr_nobs = n_sets > 0 ? n_obs : 0;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_obstacles_device(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *d_obs, void *hip_stream) {
    if (int rc = obstacles_check(ctx, n_sets, n_obs, d_obs)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_sets > 0 && n_obs > 0)      // (the caller's later work: a clearance check on its stream, which waits for the copy)
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
                HIPCHK(ctx, hipMemcpyAsync(ctx->d_clr_obs, d_obs, sizeof(mpcmp_obstacle) * n_sets * n_obs, hipMemcpyDeviceToDevice, st));
                return MPCMP_OK;
            })) return rc;
    ctx->clr_sets = n_obs > 0 ? n_sets : 0; ctx->clr_nobs = n_sets > 0 ? n_obs : 0;
    return MPCMP_OK;
}

static int clearance_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_pts, double margin, int self_gap, const mpcmp_clearance *out) {
    if (!ctx) { g_err = "mpcmp_clearance_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || n_pts < 1 || n_pts > CLR_MAX_PTS || !sx || !sT || !out || !std::isfinite(margin) || self_gap < 0) {
        ctx->err = "mpcmp_clearance_batch: B >= 1, 1 <= n_pts <= 4096, a finite margin, self_gap >= 0 and all pointers required"; return MPCMP_EINVAL;
    }
    if (ctx->clr_sets > 1 && B > ctx->clr_sets) {
        ctx->err = "more problems (" + std::to_string(B) + ") than obstacle sets (" + std::to_string(ctx->clr_sets) + "): see mpcmp_set_obstacles";
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

static int clearance_enqueue(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_pts, double margin, int self_gap,
                             mpcmp_clearance *d_out, hipStream_t st) {
    ClrTables t;
    t.d_model = ctx->d_model; t.narm = ctx->narm; t.nseg = ctx->nseg;
    t.d_sph = ctx->d_clr_sph; t.n_sph[0] = ctx->clr_nsph[0]; t.n_sph[1] = ctx->narm > 1 ? ctx->clr_nsph[1] : 0;
    t.d_obs = ctx->d_clr_obs; t.n_obs = ctx->clr_nobs; t.obs_stride = ctx->clr_sets > 1 ? ctx->clr_nobs : 0;
    if (!ctx->clr_ready) { HIPCHK(ctx, clearance_prepare()); ctx->clr_ready = true; }
    HIPCHK(ctx, clearance_launch(t, B, d_sx, d_sT, n_pts, margin, self_gap, d_out, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_pts, double margin, int self_gap,
                                            mpcmp_clearance *d_out, void *hip_stream) {
    if (int rc = clearance_check(ctx, B, d_sx, d_sT, n_pts, margin, self_gap, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return clearance_enqueue(ctx, B, d_sx, d_sT, n_pts, margin, self_gap, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_clearance_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_pts, double margin, int self_gap,
                                     mpcmp_clearance *out) {
    if (int rc = clearance_check(ctx, B, sx, sT, n_pts, margin, self_gap, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT;
    mpcmp_clearance *dout;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = clearance_enqueue(ctx, B, dx, dT, n_pts, margin, self_gap, dout, ctx->stream)) return rc;
    return sg.finish();
}

// `who`: the entry point's name; clr is required by mpcmp_select_clear_batch only
static int select_check(mpcmp_ctx *ctx, const char *who, bool need_clr, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                        const int *group, int n_groups, const int *chosen) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    if (B < 1 || n_groups < 0 || n_groups > ctx->max_batch || !sT || !info || (need_clr && !clr) || !group || (n_groups > 0 && !chosen)) {
        ctx->err = std::string(who) + ": B >= 1, n_groups in [0, max_batch] and all pointers required"; return MPCMP_EINVAL;
    }
    if (B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (!ctx->d_sel_key) {            // first use
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if (int rc = dalloc(ctx, &ctx->d_sel_key, (size_t)ctx->max_batch)) return rc;
    }
    return MPCMP_OK;
}

static int select_device(mpcmp_ctx *ctx, const char *who, bool need_clr, int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                         const mpcmp_limits *d_lim, int lim_mask, const int *d_group, int n_groups, int *d_chosen, void *hip_stream) {
    if (int rc = select_check(ctx, who, need_clr, B, d_sT, d_info, d_clr, d_group, n_groups, d_chosen)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, select_launch(B, d_sT, d_info, d_clr, d_lim, lim_mask, d_group, n_groups, ctx->d_sel_key, d_chosen, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

static int select_host(mpcmp_ctx *ctx, const char *who, bool need_clr, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                       const mpcmp_limits *lim, int lim_mask, const int *group, int n_groups, int *chosen) {
    if (int rc = select_check(ctx, who, need_clr, B, sT, info, clr, group, n_groups, chosen)) return rc;
    for (int i = 0; i < B; i++)
        if (group[i] < -1 || group[i] >= n_groups) {
            ctx->err = std::string(who) + ": group[" + std::to_string(i) + "] must be -1 or in [0, n_groups)"; return MPCMP_EINVAL;
        }
    if (n_groups == 0) return MPCMP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dT;
    mpcmp_info *di;
    mpcmp_clearance *dc;
    mpcmp_limits *dl;
    int *dg, *dch;
    sg.in(&dT, sT, B); sg.in(&di, info, B); sg.in(&dc, clr, B); sg.in(&dl, lim, B); sg.in(&dg, group, B); sg.out(&dch, chosen, n_groups);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, select_launch(B, dT, di, dc, dl, lim_mask, dg, n_groups, ctx->d_sel_key, dch, ctx->stream));
    return sg.finish();
}

extern "C" int mpcmp_select_clear_batch_device(mpcmp_ctx *ctx, int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                                               const int *d_group, int n_groups, int *d_chosen, void *hip_stream) {
    return select_device(ctx, "mpcmp_select_clear_batch", true, B, d_sT, d_info, d_clr, nullptr, 0, d_group, n_groups, d_chosen, hip_stream);
}

extern "C" int mpcmp_select_clear_batch(mpcmp_ctx *ctx, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr, const int *group,
                                        int n_groups, int *chosen) {
    return select_host(ctx, "mpcmp_select_clear_batch", true, B, sT, info, clr, nullptr, 0, group, n_groups, chosen);
}

// ------------------------------------------------------------------------------------------------
// limits between the nodes (limits.hpp; the kernel is in limits.hip)
static int limits_check(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_pts, const mpcmp_limits_spec *spec,
                        const mpcmp_limits *out) {
    if (!ctx) { g_err = "mpcmp_limits_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch || n_pts < 1 || n_pts > LIM_MAX_PTS || !sx || !su || !sT || !out) {
        ctx->err = "mpcmp_limits_batch: B in [1, max_batch], 1 <= n_pts <= 4096 and all pointers (but spec) required"; return MPCMP_EINVAL;
    }
    if (spec && !lim_spec_ok(*spec)) { ctx->err = "mpcmp_limits_batch: finite tolerances and tool maxima >= 0 (+inf: none) required"; return MPCMP_EINVAL; }
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    return rows_ok(ctx, B, PAYLOAD_ROWS);
}

static int limits_enqueue(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_pts, const mpcmp_limits_spec *spec,
                          mpcmp_limits *d_out, hipStream_t st) {
    mpcmp_bounds table;
    mpcmp_bounds_from_config(&ctx->cfg, &table);
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, limits_launch(md, ms, ctx->narm, ctx->nseg, B, n_pts, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, table, d_sx, d_su, d_sT,
                              spec ? *spec : lim_default_spec(), d_out, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_limits_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_pts,
                                         const mpcmp_limits_spec *spec, mpcmp_limits *d_out, void *hip_stream) {
    if (int rc = limits_check(ctx, B, d_sx, d_su, d_sT, n_pts, spec, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return limits_enqueue(ctx, B, d_sx, d_su, d_sT, n_pts, spec, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_limits_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_pts,
                                  const mpcmp_limits_spec *spec, mpcmp_limits *out) {
    if (int rc = limits_check(ctx, B, sx, su, sT, n_pts, spec, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t NB = (size_t)ctx->N * B;
    Stage sg(ctx);
    double *dx, *du, *dT;
    mpcmp_limits *dout;
    sg.in(&dx, sx, ctx->nx * NB); sg.in(&du, su, ctx->nu * NB); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = limits_enqueue(ctx, B, dx, du, dT, n_pts, spec, dout, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_select_checked_batch_device(mpcmp_ctx *ctx, int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                                                 const mpcmp_limits *d_lim, int lim_mask, const int *d_group, int n_groups, int *d_chosen,
                                                 void *hip_stream) {
    return select_device(ctx, "mpcmp_select_checked_batch", false, B, d_sT, d_info, d_clr, d_lim, lim_mask, d_group, n_groups, d_chosen, hip_stream);
}

extern "C" int mpcmp_select_checked_batch(mpcmp_ctx *ctx, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                                          const mpcmp_limits *lim, int lim_mask, const int *group, int n_groups, int *chosen) {
    return select_host(ctx, "mpcmp_select_checked_batch", false, B, sT, info, clr, lim, lim_mask, group, n_groups, chosen);
}

// ------------------------------------------------------------------------------------------------
// via-point routes (route.hpp, route.hip): B routes with M vias = L = B (M + 1) leg slots
// the checks every route entry point shares; *L = the number of leg slots
static int route_check(mpcmp_ctx *ctx, const char *who, int B, int M, int *L) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    if (ctx->rh_B > 0) { ctx->err = std::string(who) + ": not available after mpcmp_rh_init (the receding-horizon driver plans single moves)"; return MPCMP_EINVAL; }
    if (B < 1 || M < 0) { ctx->err = std::string(who) + ": B >= 1 and M >= 0 required"; return MPCMP_EINVAL; }
    const long long l = (long long)B * ((long long)M + 1);
    if (l > ctx->max_batch) {
        ctx->err = std::string(who) + ": " + std::to_string(l) + " leg slots (B (M + 1)) exceed the context capacity (" + std::to_string(ctx->max_batch) + ")";
        return MPCMP_EINVAL;
    }
    *L = (int)l;
    return MPCMP_OK;
}
// the host-pointer variants' look at their values: finite states and vias, speed in [0, 1]
static int route_values_ok(mpcmp_ctx *ctx, const char *who, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                           const double *xf) {
    const size_t nx = ctx->nx, nv = (size_t)B * M * (nx / 2);
    auto finite = [](const double *p, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; };
    if (!finite(x0, nx * B) || !finite(xf, nx * B) || (M > 0 && !finite(via, nv)) || (M > 0 && via_qd && !finite(via_qd, nv))) {
        ctx->err = std::string(who) + ": x0, xf, via and via_qd must be finite"; return MPCMP_EINVAL;
    }
    if (speed)
        for (int b = 0; b < B; b++)
            if (!(speed[b] >= 0.0 && speed[b] <= 1.0)) { ctx->err = std::string(who) + ": speed[" + std::to_string(b) + "] must lie in [0, 1]"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}
static int route_legs_enqueue(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                              const double *d_xf, double *d_l0, double *d_lf, double *d_vout, hipStream_t st) {
    mpcmp_bounds row;
    mpcmp_bounds_from_config(&ctx->cfg, &row);
    HIPCHK(ctx, route_legs_launch(B, M, ctx->narm, d_x0, d_via, d_vqd, d_speed, d_xf, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, row, d_l0, d_lf, d_vout, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_route_legs_device(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                                       const double *d_xf, double *d_l0, double *d_lf, double *d_vout, void *hip_stream) {
    int L;
    if (int rc = route_check(ctx, "mpcmp_route_legs", B, M, &L)) return rc;
    if (!d_x0 || !d_xf || !d_l0 || !d_lf || (M > 0 && !d_via)) { ctx->err = "mpcmp_route_legs: x0, xf, leg_x0, leg_xf (and via with M > 0) are required"; return MPCMP_EINVAL; }
    if (int rc = rows_ok(ctx, L, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return route_legs_enqueue(ctx, B, M, d_x0, d_via, d_vqd, d_speed, d_xf, d_l0, d_lf, d_vout, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_route_legs(mpcmp_ctx *ctx, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                                const double *xf, double *leg_x0, double *leg_xf, double *via_qd_out) {
    int L;
    if (int rc = route_check(ctx, "mpcmp_route_legs", B, M, &L)) return rc;
    if (!x0 || !xf || !leg_x0 || !leg_xf || (M > 0 && !via)) { ctx->err = "mpcmp_route_legs: x0, xf, leg_x0, leg_xf (and via with M > 0) are required"; return MPCMP_EINVAL; }
    if (int rc = route_values_ok(ctx, "mpcmp_route_legs", B, M, x0, via, via_qd, speed, xf)) return rc;
    if (int rc = rows_ok(ctx, L, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nx = ctx->nx, nv = (size_t)B * M * (nx / 2);
    Stage sg(ctx);
    double *d0, *df, *dv, *dq, *ds, *dl0, *dlf, *dvo;
    sg.in(&d0, x0, nx * B); sg.in(&df, xf, nx * B); sg.in(&dv, M > 0 ? via : nullptr, nv); sg.in(&dq, M > 0 ? via_qd : nullptr, nv); sg.in(&ds, speed, B);
    sg.out(&dl0, leg_x0, nx * L); sg.out(&dlf, leg_xf, nx * L); sg.out(&dvo, M > 0 ? via_qd_out : nullptr, nv);
    if (int rc = sg.upload()) return rc;
    if (int rc = route_legs_enqueue(ctx, B, M, d0, dv, dq, ds, df, dl0, dlf, dvo, ctx->stream)) return rc;
    return sg.finish();
}

static int route_join_check(mpcmp_ctx *ctx, int B, int M, const void *sx, const void *su, const void *sT, const void *info, const void *clr, const void *rT,
                            const void *rinfo, const void *seam, const void *rclr, int *L) {
    if (int rc = route_check(ctx, "mpcmp_route_join", B, M, L)) return rc;
    if (!sx || !su || !sT || !info || !rT || !rinfo || !seam || ((clr != nullptr) != (rclr != nullptr))) {
        ctx->err = "mpcmp_route_join: sol_x, sol_u, sol_T, info, route_T, route_info and seam are required; clr and route_clr both or neither"; return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_route_join_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_info *d_info,
                                       const mpcmp_clearance *d_clr, double *d_rT, mpcmp_info *d_rinfo, mpcmp_route_seam *d_seam, mpcmp_clearance *d_rclr,
                                       void *hip_stream) {
    int L;
    if (int rc = route_join_check(ctx, B, M, d_sx, d_su, d_sT, d_info, d_clr, d_rT, d_rinfo, d_seam, d_rclr, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, route_join_launch(B, M, ctx->N, ctx->narm, d_sx, d_su, d_sT, d_info, d_clr, d_rT, d_rinfo, d_seam, d_rclr, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_route_join(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, const mpcmp_info *info,
                                const mpcmp_clearance *clr, double *rT, mpcmp_info *rinfo, mpcmp_route_seam *seam, mpcmp_clearance *rclr) {
    int L;
    if (int rc = route_join_check(ctx, B, M, sx, su, sT, info, clr, rT, rinfo, seam, rclr, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t NL = (size_t)ctx->N * L;
    Stage sg(ctx);
    double *dx, *du, *dT, *drT;
    mpcmp_info *di, *dri;
    mpcmp_clearance *dc, *drc;         // (clr and rclr: both given or neither, route_join_check)
    mpcmp_route_seam *ds;
    sg.in(&dx, sx, ctx->nx * NL); sg.in(&du, su, ctx->nu * NL); sg.in(&dT, sT, L); sg.in(&di, info, L); sg.in(&dc, clr, L);
    sg.out(&drT, rT, B); sg.out(&dri, rinfo, B); sg.out(&ds, seam, B); sg.out(&drc, rclr, B);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, route_join_launch(B, M, ctx->N, ctx->narm, dx, du, dT, di, dc, drT, dri, ds, drc, ctx->stream));
    return sg.finish();
}

// everything a route solve is refused for, and its scratch (first call only)
static int route_solve_check(mpcmp_ctx *ctx, int B, int M, const void *x0, const void *via, const void *xf, const double *jmax, const void *sx, const void *su,
                             const void *sT, const void *rT, const void *rinfo, const void *seam, int *L) {
    if (int rc = route_check(ctx, "mpcmp_solve_route_batch", B, M, L)) return rc;
    if (!x0 || !xf || (M > 0 && !via) || !sx || !su || !sT || !rT || !rinfo || !seam) {
        ctx->err = "mpcmp_solve_route_batch: x0, xf (and via with M > 0), sol_x, sol_u, sol_T, route_T, route_info and seam are required"; return MPCMP_EINVAL;
    }
    if (int rc = solve_rows_ok(ctx, *L)) return rc;
    if (ctx->narm == 2 && !jmax) { ctx->err = "mpcmp_solve_route_batch: multi-arm solves need the jerk-limited start guess (jmax)"; return MPCMP_EINVAL; }
    if (jmax) { JerkLimits lim; if (int rc = jerk_limits(ctx, nullptr, nullptr, jmax, lim)) return rc; }
    if (!ctx->d_rt_x0) {              // first use
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const size_t Mx = ctx->max_batch, N = ctx->N, nx = ctx->nx, nu = ctx->nu;
        if (int rc = dalloc(ctx, &ctx->d_rt_xf, Mx * nx)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_wx, Mx * nx * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_wu, Mx * nu * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_wT, Mx)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_info, Mx)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_x0, Mx * nx)) return rc;      // (last: the mark of a complete scratch)
    }
    return MPCMP_OK;
}

// leg builder, start guess, one solve of the L legs, join: all on st, no host round trip
static int route_solve_enqueue(mpcmp_ctx *ctx, int B, int M, int L, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                               const double *d_xf, const double *jmax, double *d_sx, double *d_su, double *d_sT, mpcmp_info *d_info, double *d_rT,
                               mpcmp_info *d_rinfo, mpcmp_route_seam *d_seam, double *d_vout, hipStream_t st) {
    if (int rc = route_legs_enqueue(ctx, B, M, d_x0, d_via, d_vqd, d_speed, d_xf, ctx->d_rt_x0, ctx->d_rt_xf, d_vout, st)) return rc;
    SolveCall c;
    c.B = L; c.x0 = ctx->d_rt_x0; c.xf = ctx->d_rt_xf;
    if (jmax) {
        if (int rc = mpcmp_warm_start_jerk_batch_device(ctx, L, ctx->d_rt_x0, ctx->d_rt_xf, jmax, ctx->d_rt_wx, ctx->d_rt_wu, ctx->d_rt_wT, st)) return rc;
        c.wx = ctx->d_rt_wx; c.wu = ctx->d_rt_wu; c.wT = ctx->d_rt_wT;
    }
    c.sx = d_sx; c.su = d_su; c.sT = d_sT; c.info = d_info ? d_info : ctx->d_rt_info; c.stream = st;
    if (int rc = solve_dispatch(ctx, c)) return rc;
    HIPCHK(ctx, route_join_launch(B, M, ctx->N, ctx->narm, d_sx, d_su, d_sT, c.info, nullptr, d_rT, d_rinfo, d_seam, nullptr, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_solve_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                                              const double *d_xf, const double *jmax, double *d_sx, double *d_su, double *d_sT, mpcmp_info *d_info,
                                              double *d_rT, mpcmp_info *d_rinfo, mpcmp_route_seam *d_seam, double *d_vout, void *hip_stream) {
    int L;
    if (int rc = route_solve_check(ctx, B, M, d_x0, d_via, d_xf, jmax, d_sx, d_su, d_sT, d_rT, d_rinfo, d_seam, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return route_solve_enqueue(ctx, B, M, L, d_x0, d_via, d_vqd, d_speed, d_xf, jmax, d_sx, d_su, d_sT, d_info, d_rT, d_rinfo, d_seam, d_vout,
                               (hipStream_t)hip_stream);
}

extern "C" int mpcmp_solve_route_batch(mpcmp_ctx *ctx, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                                       const double *xf, const double *jmax, double *sx, double *su, double *sT, mpcmp_info *info, double *rT,
                                       mpcmp_info *rinfo, mpcmp_route_seam *seam, double *via_qd_out) {
    int L;
    if (int rc = route_check(ctx, "mpcmp_solve_route_batch", B, M, &L)) return rc;
    if (!x0 || !xf || (M > 0 && !via)) { ctx->err = "mpcmp_solve_route_batch: x0, xf (and via with M > 0) are required"; return MPCMP_EINVAL; }
    if (int rc = route_values_ok(ctx, "mpcmp_solve_route_batch", B, M, x0, via, via_qd, speed, xf)) return rc;
    if (int rc = route_solve_check(ctx, B, M, x0, via, xf, jmax, sx, su, sT, rT, rinfo, seam, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nx = ctx->nx, nv = (size_t)B * M * (nx / 2);
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *d0, *df, *dv, *dq, *ds, *drT, *dvo;
    mpcmp_info *dri;
    mpcmp_route_seam *dsm;
    sg.in(&d0, x0, nx * B); sg.in(&df, xf, nx * B); sg.in(&dv, M > 0 ? via : nullptr, nv); sg.in(&dq, M > 0 ? via_qd : nullptr, nv); sg.in(&ds, speed, B);
    sg.out(&drT, rT, B); sg.out(&dri, rinfo, B); sg.out(&dsm, seam, B); sg.out(&dvo, M > 0 ? via_qd_out : nullptr, nv);
    if (int rc = sg.upload()) return rc;
    if (int rc = route_solve_enqueue(ctx, B, M, L, d0, dv, dq, ds, df, jmax, ctx->d_sx, ctx->d_su, ctx->d_sT, ctx->d_info, drT, dri, dsm, dvo, st)) return rc;
    if (int rc = download_trajectories(ctx, L, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    return sg.finish();
}

static int route_sample_check(mpcmp_ctx *ctx, int B, int M, const void *sx, const void *su, const void *sT, int n_pts, const void *out, int *L) {
    if (int rc = route_check(ctx, "mpcmp_sample_route_batch", B, M, L)) return rc;
    if (n_pts < 1 || !sx || !su || !sT || !out) { ctx->err = "mpcmp_sample_route_batch: n_pts >= 1 and all pointers required"; return MPCMP_EINVAL; }
    SINGLE_ARM_ONLY(ctx);
    return rows_ok(ctx, *L, PAYLOAD_ROWS);
}

extern "C" int mpcmp_sample_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, int n_pts,
                                               double *d_out, void *hip_stream) {
    int L;
    if (int rc = route_sample_check(ctx, B, M, d_sx, d_su, d_sT, n_pts, d_out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, route_sample_launch(md, ms, ctx->nseg, B, M, n_pts, d_sx, d_su, d_sT, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_sample_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_pts, double *out) {
    int L;
    if (int rc = route_sample_check(ctx, B, M, sx, su, sT, n_pts, out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t NL = (size_t)ctx->N * L;
    Stage sg(ctx);
    double *dx, *du, *dT, *dout;
    sg.in(&dx, sx, 14 * NL); sg.in(&du, su, 7 * NL); sg.in(&dT, sT, L); sg.out(&dout, out, (size_t)B * (n_pts + 1) * 29);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sample_route_batch_device(ctx, B, M, dx, du, dT, n_pts, dout, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// batched tool-pose targets (ik_device.hpp): B problems x S starts of the DLS inverse kinematics, one start chosen per problem, xf columns of one arm
static int pose_targets_check(mpcmp_ctx *ctx, int B, int arm, const double *R, const double *p, int S, const double *seeds, const double *xf) {
    if (!ctx) { g_err = "mpcmp_pose_targets: no context"; return MPCMP_EINVAL; }
    if (B < 1) { ctx->err = "mpcmp_pose_targets: B must be >= 1"; return MPCMP_EINVAL; }
    if (S < 1 || S > 64) { ctx->err = "mpcmp_pose_targets: S must be in [1, 64]"; return MPCMP_EINVAL; }
    if (arm < 0 || arm >= ctx->narm) { ctx->err = "mpcmp_pose_targets: arm must be in [0, narm)"; return MPCMP_EINVAL; }
    if (!R || !p || !seeds || !xf) { ctx->err = "mpcmp_pose_targets: R, p, q_seeds and xf are required"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

extern "C" int mpcmp_pose_targets_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_R, const double *d_p, const double *d_twist,
                                               int S, const double *d_seeds, const double *d_q_ref, double *d_xf, mpcmp_ik_info *d_info, void *hip_stream) {
    if (int rc = pose_targets_check(ctx, B, arm, d_R, d_p, S, d_seeds, d_xf)) return rc;
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IkBounds bd;
    for (int j = 0; j < 7; j++) { bd.lq[j] = ctx->cfg.lbx[j]; bd.uq[j] = ctx->cfg.ubx[j]; bd.lv[j] = ctx->cfg.lbx[7 + j]; bd.uv[j] = ctx->cfg.ubx[7 + j]; }
    int P = 1;
    while (P < S) P <<= 1;
    const long threads = (long)B * P;
    hipLaunchKernelGGL(k_pose_targets, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, ctx->d_model + arm, bd, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, B, S, P,
                       ctx->nx, 7 * arm, 7 * ctx->narm + 7 * arm, d_R, d_p, d_twist, d_seeds, d_q_ref, d_xf, d_info);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_pose_targets_batch(mpcmp_ctx *ctx, int B, int arm, const double *R, const double *p, const double *twist,
                                        int S, const double *seeds, const double *q_ref, double *xf, mpcmp_ik_info *info) {
    if (int rc = pose_targets_check(ctx, B, arm, R, p, S, seeds, xf)) return rc;
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    const size_t nb = B, nx = ctx->nx;
    const struct { const double *v; size_t n; } in[5] = {{R, 9 * nb}, {p, 3 * nb}, {twist, 6 * nb}, {seeds, 7 * nb * S}, {q_ref, 7 * nb}};
    for (const auto &a : in)
        if (a.v)
            for (size_t k = 0; k < a.n; k++)
                if (!std::isfinite(a.v[k])) { ctx->err = "mpcmp_pose_targets: an input value is not finite"; return MPCMP_EINVAL; }
    for (size_t b = 0; b < nb; b++) {
        const double *r = R + 9 * b;
        double dev = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double g = r[i] * r[j] + r[3 + i] * r[3 + j] + r[6 + i] * r[6 + j] - (i == j ? 1.0 : 0.0);
                dev = std::max(dev, std::fabs(g));
            }
        const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
        if (dev > 1e-6 || !(det > 0.0)) {
            std::ostringstream os;
            os << "mpcmp_pose_targets: R of problem " << b << " is not a rotation";
            ctx->err = os.str();
            return MPCMP_EINVAL;
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dR, *dp_, *dtw, *dsd, *dqr, *dxf;
    mpcmp_ik_info *dinfo;
    sg.in(&dR, R, 9 * nb); sg.in(&dp_, p, 3 * nb); sg.in(&dtw, twist, 6 * nb); sg.in(&dsd, seeds, 7 * nb * S); sg.in(&dqr, q_ref, 7 * nb);
    sg.inout(&dxf, xf, nx * nb);       // the other arm's columns come back as they were
    sg.out(&dinfo, info, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_pose_targets_batch_device(ctx, B, arm, dR, dp_, dtw, S, dsd, dqr, dxf, dinfo, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// receding-horizon driver (BASELINE config #5): B instances, every step = warm-started re-solve from the previous
// solution (re-guess rule of motionPlanner.cpp:199-207) + state advance along the new solution
// (get_MPC_point, motionPlanner.hpp:118-128).  The fixed launch sequence of one step is captured in a hipGraph.
extern "C" int mpcmp_reset_multipliers(mpcmp_ctx *ctx) {
    if (!ctx) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.lam, 0, sizeof(double) * ctx->lam_count, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.status, 0, sizeof(*ctx->ws.status) * ctx->max_batch, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_init(mpcmp_ctx *ctx, int B, const double *x0, const double *xf) {
    if (!ctx || !x0 || !xf || B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    if (ctx->bnd_rows > 0) { ctx->err = "mpcmp_rh_init: the receding-horizon driver does not read bound rows (clear them: mpcmp_set_bounds(ctx, 0, NULL))"; return MPCMP_EINVAL; }
    if (ctx->tw_rows > 0) { ctx->err = "mpcmp_rh_init: the receding-horizon driver does not read final-time rows (clear them: mpcmp_set_time_windows(ctx, 0, NULL, NULL))"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.lam, 0, sizeof(double) * ctx->lam_count, st));       // new instances: no multipliers to carry, no failed solve behind them
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.status, 0, sizeof(*ctx->ws.status) * ctx->max_batch, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_retired, 0, sizeof(int) * ctx->max_batch, st));                       // nobody has arrived
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rh_count, 0, 2 * sizeof(unsigned long long), st));
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->rh_B = B; ctx->rh_first = true;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

// capturing: st is being captured into the step graph
static int rh_enqueue_step(mpcmp_ctx *ctx, double dt, bool first, hipStream_t st, bool capturing) {
    const int B = ctx->rh_B;
    // The driver's start guess, every step, from every instance's current state: the jerk-limited time-synchronised trajectory the reference takes from
    // Ruckig for solve_trajectory(true) (motionPlanner.cpp:146-175), with the velocity / acceleration limits of the configuration and the jerk
    // margin every example of the reference uses (0.1 x max jerk: examples/offline_trajectory.cpp:9, benchmark.cpp).  It starts the first solve and
    // RE-starts an instance whose previous solve is no guess (hard failure, T outside its box, or a restart asked for by mpcmp_rh_update: k_init); the
    // other re-solves re-guess from the previous solution (solve_trajectory(false), motionPlanner.cpp:199-207).
    double jm[7];
    mpcmp_default_limits(nullptr, nullptr, nullptr, nullptr, jm, nullptr);
    for (int j = 0; j < 7; j++) jm[j] *= 0.1;
    // (after the first step only for the instances that restart: the generator costs ~ 0.15 ms per 512 instances, 4 % of a step)
    if (int rc = warm_start_jerk_device(ctx, B, ctx->d_x0, ctx->d_xf, nullptr, nullptr, nullptr, nullptr, jm, ctx->d_wx, ctx->d_wu, ctx->d_wT, st,
                                        first ? nullptr : ctx->ws.status, MPCMP_ST_NO_GUESS))
        return rc;
    SolveCall c = staged_call(ctx, B, true, st);
    if (!first) { c.wx = ctx->d_sx; c.wu = ctx->d_su; c.wT = ctx->d_sT; c.reguess = 1; }
    c.rh_step = true;              // the driver's defaults of the start flags (run_config) and the retired instances (WS::retired)
    c.capturing = capturing;
    if (int rc = solve_dispatch(ctx, c)) return rc;
    hipLaunchKernelGGL(k_advance, dim3((B + 255) / 256), dim3(256), 0, st, ctx->nseg, ctx->nx, B, dt, ctx->cfg.eps_target, ctx->d_sx, ctx->d_sT,
                       ctx->ws.status, ctx->d_xf, ctx->d_x0, ctx->d_retired, ctx->d_info, ctx->d_rh_count);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_run(mpcmp_ctx *ctx, int steps, double dt, int use_graph) {
    if (!ctx || steps < 1 || !(dt > 0.0) || ctx->rh_B < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int done = 0;
    if (ctx->rh_first) {                       // first solve: built-in initialiser, not part of the graph
        if (int rc = rh_enqueue_step(ctx, dt, true, st, false)) return rc;
        ctx->rh_first = false; done = 1;
    }
    if (use_graph && steps - done > 0) {
        if (!ctx->rh_exec || ctx->rh_dt != dt) {
            drop_rh_graph(ctx);
            HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            const int rc = rh_enqueue_step(ctx, dt, false, st, true);
            hipError_t e = hipStreamEndCapture(st, &ctx->rh_graph);
            if (rc) return rc;
            HIPCHK(ctx, e);
            HIPCHK(ctx, hipGraphInstantiate(&ctx->rh_exec, ctx->rh_graph, nullptr, nullptr, 0));
            ctx->rh_dt = dt;
        }
        for (; done < steps; done++) HIPCHK(ctx, hipGraphLaunch(ctx->rh_exec, st));
    } else {
        for (; done < steps; done++)
            if (int rc = rh_enqueue_step(ctx, dt, false, st, false)) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

// Between two steps: new measured states and / or targets of listed instances (k_rh_update).  Only buffer contents change: a captured step graph
// stays valid, and the next step reads the new values through the pointers it was captured with.
static int rh_update_check(mpcmp_ctx *ctx, int n, const int *idx, const double *x, const double *xf, int flags) {
    if (!ctx) { g_err = "mpcmp_rh_update: no context"; return MPCMP_EINVAL; }
    if (ctx->rh_B < 1) { ctx->err = "mpcmp_rh_update: no receding-horizon loop (mpcmp_rh_init first)"; return MPCMP_EINVAL; }
    if (n < 1 || n > ctx->rh_B) { ctx->err = "mpcmp_rh_update: n must be in [1, B] of mpcmp_rh_init"; return MPCMP_EINVAL; }
    if (!idx && n != ctx->rh_B) { ctx->err = "mpcmp_rh_update: idx NULL needs n == B"; return MPCMP_EINVAL; }
    if (!x && !xf) { ctx->err = "mpcmp_rh_update: x and xf are both NULL"; return MPCMP_EINVAL; }
    if (flags & ~MPCMP_RH_RESTART) { ctx->err = "mpcmp_rh_update: unknown flag bits"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

static int rh_update_enqueue(mpcmp_ctx *ctx, int n, const int *d_idx, const double *d_x, const double *d_xf, int flags, hipStream_t st) {
    hipLaunchKernelGGL(k_rh_update, dim3((n + 255) / 256), dim3(256), 0, st, ctx->nx, n, d_idx, d_x, d_xf, (flags & MPCMP_RH_RESTART) ? 1 : 0,
                       ctx->d_x0, ctx->d_xf, ctx->d_retired, ctx->ws.status, ctx->d_info, ctx->d_rh_count);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_update(mpcmp_ctx *ctx, int n, const int *idx, const double *x, const double *xf, int flags) {
    if (int rc = rh_update_check(ctx, n, idx, x, xf, flags)) return rc;
    const int B = ctx->rh_B;
    const size_t nx = ctx->nx;
    if (idx) {
        std::vector<char> seen(B, 0);
        for (int i = 0; i < n; i++) {
            if (idx[i] < 0 || idx[i] >= B) { ctx->err = "mpcmp_rh_update: instance index out of range"; return MPCMP_EINVAL; }
            if (seen[idx[i]]++) { ctx->err = "mpcmp_rh_update: instance index repeated"; return MPCMP_EINVAL; }
        }
    }
    for (const double *v : {x, xf})
        if (v)
            for (size_t k = 0; k < n * nx; k++)
                if (!std::isfinite(v[k])) { ctx->err = "mpcmp_rh_update: a state or target value is not finite"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    int *di;
    double *dx, *dxf;
    sg.in(&di, idx, n); sg.in(&dx, x, n * nx); sg.in(&dxf, xf, n * nx);
    if (int rc = sg.upload()) return rc;
    if (int rc = rh_update_enqueue(ctx, n, di, dx, dxf, flags, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_rh_update_device(mpcmp_ctx *ctx, int n, const int *d_idx, const double *d_x, const double *d_xf, int flags, void *hip_stream) {
    if (int rc = rh_update_check(ctx, n, d_idx, d_x, d_xf, flags)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return with_caller_stream(ctx, hip_stream, [&](hipStream_t st) { return rh_update_enqueue(ctx, n, d_idx, d_x, d_xf, flags, st); });
}

extern "C" int mpcmp_rh_get(mpcmp_ctx *ctx, double *x0_now, double *sx, double *su, double *sT, mpcmp_info *info) {
    if (!ctx || ctx->rh_B < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t B = ctx->rh_B;
    hipStream_t st = ctx->stream;
    if (x0_now) HIPCHK(ctx, hipMemcpyAsync(x0_now, ctx->d_x0, sizeof(double) * ctx->nx * B, hipMemcpyDeviceToHost, st));
    if (int rc = download_trajectories(ctx, B, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_stats(mpcmp_ctx *ctx, long long *resolves_done, long long *arrived) {
    if (!ctx || ctx->rh_B < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long c[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(c, ctx->d_rh_count, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (resolves_done) *resolves_done = (long long)c[0];
    if (arrived) *arrived = (long long)c[1];
    return MPCMP_OK;
}

// diagnostics: copy one workspace array of the last solve to the host (which: 0 z, 1 lambda, 2 c_eq, 3 g, 4 p, 5 y)
extern "C" int mpcmp_debug_fetch(mpcmp_ctx *ctx, int which, double *out, long count) {
    if (!ctx || !out || count < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const double *src = which == 0 ? ctx->ws.z : which == 1 ? ctx->ws.lam : which == 2 ? ctx->ws.ceq : which == 3 ? ctx->ws.g
                      : which == 4 ? ctx->ws.p : which == 5 ? ctx->ws.y : nullptr;
    if (!src) return MPCMP_EINVAL;
    HIPCHK(ctx, hipMemcpy(out, src, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return MPCMP_OK;
}

// diagnostics: raw phase stamps of the last k_qp launch (all zero unless built with -DMPCMP_STAMPS)
extern "C" int mpcmp_debug_stamps(mpcmp_ctx *ctx, int B, unsigned long long *out) {
    if (!ctx || !out || B < 1 || B > ctx->max_batch) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(out, ctx->ws.dbg, sizeof(unsigned long long) * MPCMP_DBG_WORDS * B, hipMemcpyDeviceToHost));
    return MPCMP_OK;
}

extern "C" int mpcmp_kernel_timing(mpcmp_ctx *ctx, int reset, const char **name, double *ms_total, int *launches) {
    if (!ctx) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // fold finished event pairs into the accumulators (caller has synchronised the stream)
    for (size_t i = 0; i < ctx->ev_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev[i].e[0], ctx->ev[i].e[1]) == hipSuccess) { ctx->qp_ms += ms; ctx->qp_launches++; }
    }
    ctx->ev_used = 0;
    ctx->timing = true;            // event recording starts with the first call (bench.py calls it once before the timed region)
    if (name) *name = ctx->loop_kernel;
    if (ms_total) *ms_total = ctx->qp_ms;
    if (launches) *launches = ctx->qp_launches;
    if (reset) { ctx->qp_ms = 0.0; ctx->qp_launches = 0; }
    return MPCMP_OK;
}
